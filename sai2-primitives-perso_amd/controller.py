"""Host-side mirror of the reference's controller interface over the C ABI (include/sai2b.h).

``Controller`` is the thin array-level binding (SoA numpy arrays or raw device pointers in, torques
out). The classes ``BatchedRobotModel``, ``JointTask``, ``MotionForceTask`` and ``RobotController``
keep the reference's names, argument meaning and error behaviour
(reference src/RobotController.h:25-40, src/tasks/JointTask.h:56-384,
src/tasks/MotionForceTask.h:96-753) but every vector/matrix is batched: shape ``[C, B]``
(component-major, batch-minor). std::invalid_argument becomes ValueError; HIP failures RuntimeError.

All numerical work happens in csrc/libsai2b.so (HIP, gfx950). There is no CPU fallback: creating a
controller without the library or without a GPU raises.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import DOF, MOTION_FORCE_TASK, RobotModel, TaskConfig
from .workloads import EE_FRAME_POS, EE_LINK


def _check(lib, handle, rc):
    if rc == _abi.OK:
        return
    msg = lib.sai2b_last_error(handle)
    msg = msg.decode() if msg else "unknown error"
    if rc == _abi.INVALID_ARGUMENT:
        raise ValueError(msg)
    raise RuntimeError(msg)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def panda_model():
    """sai2b_panda_model(): Panda constants with the fixed end-effector body merged into link 7."""
    lib = _abi.load_library()
    m = RobotModel()
    _check(lib, None, lib.sai2b_panda_model(C.byref(m)))
    return m


def model_from_urdf(urdf, is_file=True):
    """sai2b_model_from_urdf(): (RobotModel, UrdfLinks) from a URDF file name or XML text"""
    lib = _abi.load_library()
    m, links = RobotModel(), _abi.UrdfLinks()
    _check(lib, None, lib.sai2b_model_from_urdf(urdf.encode(), 1 if is_file else 0, C.byref(m), C.byref(links)))
    return m, links


def with_base_transform(model, pos, rot=None):
    """sai2b_model_set_base_transform() on a COPY of the model: Sai2Model::setTRobotBase (examples/05-...cpp:69).
    The tasks work in the world frame (MotionForceTask.cpp:100-103, 262: positionInWorld / JWorldFrame), so the base
    pose is part of the model a Controller is built from."""
    lib = _abi.load_library()
    m = RobotModel()
    C.memmove(C.byref(m), C.byref(model), C.sizeof(RobotModel))
    p = np.ascontiguousarray(pos, dtype=np.float64).reshape(3)
    r = None if rot is None else np.ascontiguousarray(rot, dtype=np.float64).reshape(9)
    _check(lib, None, lib.sai2b_model_set_base_transform(C.byref(m), _dp(p), _dp(r)))
    return m


def resolve_link_frame(links, link_name, pos_in_link=(0.0, 0.0, 0.0), rot_in_link=None):
    """sai2b_urdf_resolve_frame(): link name + frame in that link -> (moving link index, frame_pos, frame_rot)"""
    lib = _abi.load_library()
    p = np.ascontiguousarray(pos_in_link, dtype=np.float64)
    r = None if rot_in_link is None else np.ascontiguousarray(rot_in_link, dtype=np.float64)
    link, fp, fr = C.c_int(), np.zeros(3), np.zeros(9)
    _check(lib, None, lib.sai2b_urdf_resolve_frame(C.byref(links), link_name.encode(), _dp(p), _dp(r), C.byref(link), _dp(fp), _dp(fr)))
    return link.value, fp, fr.reshape(3, 3)


def joint_task_config(name=None, selection=None, internal_otg=False, robot_dof=DOF):
    """sai2b_default_joint_task(): JointTask ctor + defaults (JointTask.cpp:14-89).
    The library default is the reference's: internal OTG on (JointTask.h:38). This helper turns it
    off unless internal_otg=True, the way the reference's examples call disableInternalOtg() after
    construction (examples/05-...cpp:117) and as BASELINE's workloads are defined."""
    lib = _abi.load_library()
    c = TaskConfig()
    sel = None if selection is None else np.ascontiguousarray(selection, dtype=np.float64)
    if sel is not None and (sel.ndim != 2 or sel.shape[1] != robot_dof):
        raise ValueError("joint selection matrix size not consistent with robot dof in JointTask constructor\n")
    rc = lib.sai2b_default_joint_task_dof(C.byref(c), name.encode() if name else None, int(robot_dof), 0 if sel is None else sel.shape[0],
                                          _dp(sel))
    _check(lib, None, rc)
    if not internal_otg:
        c.use_internal_otg = 0
    return c


def motion_force_task_config(name=None, link=EE_LINK, frame_pos=EE_FRAME_POS, frame_rot=None, partial=None,
                             internal_otg=False, robot_dof=DOF):
    """sai2b_default_motion_force_task(): MotionForceTask ctors + defaults (MotionForceTask.cpp:16-202).
    partial = (translation directions [n,3], rotation directions [m,3]) selects the partial-task ctor.
    internal_otg: see joint_task_config (library default on, this helper's default off)."""
    lib = _abi.load_library()
    c = TaskConfig()
    fp = np.ascontiguousarray(frame_pos, dtype=np.float64)
    fr = None if frame_rot is None else np.ascontiguousarray(frame_rot, dtype=np.float64)
    if partial is None:
        nt, nr, dt, dr = -1, -1, None, None
    else:
        dt = np.ascontiguousarray(partial[0], dtype=np.float64).reshape(-1, 3)
        dr = np.ascontiguousarray(partial[1], dtype=np.float64).reshape(-1, 3)
        nt, nr = dt.shape[0], dr.shape[0]
    rc = lib.sai2b_default_motion_force_task_dof(
        C.byref(c), name.encode() if name else None, int(robot_dof), link, _dp(fp), _dp(fr),
        nt, _dp(dt) if nt and nt > 0 else None, nr, _dp(dr) if nr and nr > 0 else None,
    )
    _check(lib, None, rc)
    if not internal_otg:
        c.use_internal_otg = 0
    return c


def task_configs(tasks):
    """workloads.make_inputs()['tasks'] -> list of TaskConfig built by the product's helpers"""
    out = []
    for t, (kind, prm) in enumerate(tasks):
        if kind == "jt":
            out.append(joint_task_config(f"joint_task_{t}", prm.get("selection")))
        else:
            out.append(motion_force_task_config(f"motion_force_task_{t}", partial=prm.get("partial")))
    return out


def body_contact_config(robot_dof, categories=("plane", "obstacle", "self"), v_eps=1e-3):
    """sai2b_default_body_contact() + sai2b_validate_body_contact() for a robot of robot_dof joints (no device needed) ->
    BodyContactConfig. categories: names of _abi.COL_CATEGORIES (or an int of bits 1 << category); v_eps: the friction
    regularisation (m/s)."""
    lib = _abi.load_library()
    cfg = _abi.BodyContactConfig()
    if lib.sai2b_default_body_contact(C.byref(cfg)):
        raise ValueError(lib.sai2b_last_error(None).decode())
    if isinstance(categories, (int, np.integer)):
        cfg.categories = int(categories)
    else:
        bits = 0
        for name in ([categories] if isinstance(categories, str) else categories):
            if name not in _abi.COL_CATEGORIES:
                raise ValueError(f"unknown body contact category {name!r} (one of {_abi.COL_CATEGORIES})")
            bits |= 1 << _abi.COL_CATEGORIES.index(name)
        cfg.categories = bits
    cfg.v_eps = float(v_eps)
    msg = C.create_string_buffer(256)
    if lib.sai2b_validate_body_contact(C.byref(cfg), int(robot_dof), msg, 256):
        raise ValueError(msg.value.decode())
    return cfg


def collision_config(robot_dof, links, centres, radii, n_planes=0, n_obstacles=0, blocks=("distance",), margin_plane=0.0, margin_obstacle=0.0,
                     margin_self=0.0, view="truth", env_mask=None, pairs="default"):
    """sai2b_default_collision() + sai2b_validate_collision() for a robot of robot_dof joints (no device needed) -> CollisionConfig.
    links [n]: moving-link index of every sphere, -1 = the world; centres [n][3] in the link's
    frame; radii [n]. blocks: names of _abi.COL_BLOCKS ('distance', 'index', 'normal', 'gradient', 'centres'). view: 'truth' or
    'measured' (or 0 / 1). env_mask: None = the default (every sphere on a moving link), or an int of bits, or the sphere
    indices. pairs: 'default' (links at least 2 apart), 'all', 'none', or an iterable of (i, j) with i < j."""
    links = np.ascontiguousarray(links, dtype=np.int32).reshape(-1)
    n = links.shape[0]
    centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
    radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (n,)))
    if centres.shape[0] != n:
        raise ValueError("collision: one centre per sphere is required")
    lib = _abi.load_library()
    cfg = _abi.CollisionConfig()
    if lib.sai2b_default_collision(C.byref(cfg), n, C.c_void_p(links.ctypes.data), C.c_void_p(centres.ctypes.data), C.c_void_p(radii.ctypes.data)):
        raise ValueError(lib.sai2b_last_error(None).decode())
    cfg.n_planes, cfg.n_obstacles = int(n_planes), int(n_obstacles)
    cfg.blocks = Controller._flags(blocks, _abi.COL_BLOCKS, "collision block")
    cfg.margin_plane, cfg.margin_obstacle, cfg.margin_self = float(margin_plane), float(margin_obstacle), float(margin_self)
    if isinstance(view, str):
        if view not in ("truth", "measured"):
            raise ValueError("view must be 'truth' or 'measured'")
        view = 0 if view == "truth" else 1
    cfg.view = int(view)
    if env_mask is not None:
        cfg.env_mask = int(env_mask) if isinstance(env_mask, (int, np.integer)) else sum({1 << int(k) for k in env_mask})
    if not (isinstance(pairs, str) and pairs == "default"):
        for i in range(16):
            cfg.pair_mask[i] = 0
        if isinstance(pairs, str):
            if pairs not in ("all", "none"):
                raise ValueError("pairs must be 'default', 'all', 'none' or an iterable of (i, j)")
            if pairs == "all":
                for i in range(n):
                    cfg.pair_mask[i] = ((1 << n) - 1) & ~((2 << i) - 1)
        else:
            for i, j in pairs:
                if not 0 <= int(i) < 16 or not 0 <= int(j) < 32:
                    raise ValueError(f"collision: pair ({i}, {j}) out of range")
                cfg.pair_mask[int(i)] |= 1 << int(j)
    msg = C.create_string_buffer(256)
    if lib.sai2b_validate_collision(C.byref(cfg), int(robot_dof), msg, 256):
        raise ValueError(msg.value.decode())
    return cfg



def ik_config(model, task=0, axes=0b111111, rot_length=0.25, max_iterations=40, restarts=0, tol_pos=1e-6, tol_rot=1e-6, mu0=1e-2, mu_min=1e-9,
              mu_max=1e3, mu_down=0.25, mu_up=8.0, step_max=0.5, use_limits=True, limit_margin=0.0, rest_weight=0.0, view="truth",
              goal_source="rows", seed_source="rows", seed=0, first_robot=0, draw_id=0):
    """sai2b_default_ik() + sai2b_validate_ik() against a RobotModel's size and limits (no device needed) -> IkConfig. axes: an int of bits or an iterable of 'x', 'y', 'z', 'wx', 'wy',
    'wz'; view: 'truth' or 'measured'; goal_source: 'rows' or 'task'; seed_source: 'rows' or 'state'"""
    lib, dof = _abi.load_library(), int(model.dof)
    cfg = _abi.IkConfig()
    if lib.sai2b_default_ik(C.byref(cfg)):
        raise ValueError(lib.sai2b_last_error(None).decode())
    names = ("x", "y", "z", "wx", "wy", "wz")
    try:
        cfg.axes = int(axes) if isinstance(axes, (int, np.integer)) else sum({1 << names.index(a) for a in axes})
        cfg.view = {"truth": 0, "measured": 1}[view] if isinstance(view, str) else int(view)
        cfg.goal_source = {"rows": _abi.IK_ROWS, "task": _abi.IK_TASK_GOAL}[goal_source] if isinstance(goal_source, str) else int(goal_source)
        cfg.seed_source = {"rows": _abi.IK_ROWS, "state": _abi.IK_STATE}[seed_source] if isinstance(seed_source, str) else int(seed_source)
    except (KeyError, ValueError):
        raise ValueError("ik: axes are 'x', 'y', 'z', 'wx', 'wy', 'wz'; view 'truth' or 'measured'; goal_source 'rows' or 'task'; "
                         "seed_source 'rows' or 'state'") from None
    cfg.task, cfg.max_iterations, cfg.restarts, cfg.use_limits = int(task), int(max_iterations), int(restarts), int(bool(use_limits))
    cfg.rot_length, cfg.tol_pos, cfg.tol_rot = float(rot_length), float(tol_pos), float(tol_rot)
    cfg.mu0, cfg.mu_min, cfg.mu_max, cfg.mu_down, cfg.mu_up = float(mu0), float(mu_min), float(mu_max), float(mu_down), float(mu_up)
    cfg.step_max, cfg.limit_margin, cfg.rest_weight = float(step_max), float(limit_margin), float(rest_weight)
    cfg.seed, cfg.first_robot, cfg.draw_id = int(seed), int(first_robot), int(draw_id)
    lo = np.array(model.q_lower[: dof], dtype=np.float64)
    hi = np.array(model.q_upper[: dof], dtype=np.float64)
    msg = C.create_string_buffer(256)
    if lib.sai2b_validate_ik(C.byref(cfg), dof, C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data), msg, 256):
        raise ValueError(msg.value.decode())
    return cfg


class Controller:
    """Array-level binding of one sai2b_ctx (one GPU, one batch)."""

    def __init__(self, model, tasks, batch, device=0, introspection=False):
        self.lib = _abi.load_library()
        self.B = int(batch)
        self.dof = int(model.dof)  # joints of the robot: the library routes to its build for that size
        self.model = model
        self.tasks = list(tasks)
        arr = (TaskConfig * len(self.tasks))(*self.tasks)
        self.h = self.lib.sai2b_create(C.byref(model), arr, len(self.tasks), self.B, int(device))
        if not self.h:
            msg = self.lib.sai2b_last_error(None).decode()
            if "hip" in msg.lower():
                raise RuntimeError(msg)
            raise ValueError(msg)
        self._caller_stream = 0  # the legacy default stream
        self._device = int(device)
        if introspection:
            self.enable_introspection(True)

    # -- lifetime
    def close(self):
        if getattr(self, "h", None):
            self.lib.sai2b_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rc(self, rc):
        _check(self.lib, self.h, rc)

    def _in(self, a, rows):
        """-> (pointer, on_device, keepalive) for a numpy array, a torch CUDA tensor, or None"""
        if a is None:
            return None, None
        if hasattr(a, "data_ptr"):  # torch tensor
            if not a.is_cuda or not a.is_contiguous() or tuple(a.shape) != (rows, self.B) or str(a.dtype) != "torch.float64":
                raise ValueError(f"expected a contiguous float64 CUDA tensor of shape ({rows}, {self.B})")
            # the tensor was (or is being) produced on torch's current stream: sai2b.h "stream contract"
            import torch

            s = torch.cuda.current_stream(a.device).cuda_stream
            if s != self._caller_stream:
                self._rc(self.lib.sai2b_set_caller_stream(self.h, C.c_void_p(s)))
                self._caller_stream = s
            return C.c_void_p(a.data_ptr()), a
        arr = np.ascontiguousarray(a, dtype=np.float64)
        if arr.shape != (rows, self.B):
            raise ValueError(f"expected an array of shape ({rows}, {self.B}), got {arr.shape}")
        return C.c_void_p(arr.ctypes.data), arr

    @staticmethod
    def _dev(*objs):
        kinds = {hasattr(o, "data_ptr") for o in objs if o is not None}
        if len(kinds) > 1:
            raise ValueError("mixing host arrays and device tensors in one call")
        return 1 if kinds == {True} else 0

    # -- configuration
    def update_task_config(self, task, cfg):
        self._rc(self.lib.sai2b_update_task_config(self.h, task, C.byref(cfg)))
        self.tasks[task] = cfg

    def enable_gravity_compensation(self, on=True):
        self._rc(self.lib.sai2b_enable_gravity_compensation(self.h, int(on)))

    def enable_introspection(self, on=True):
        self._rc(self.lib.sai2b_enable_introspection(self.h, int(on)))

    # -- inputs
    def set_state(self, q=None, dq=None):
        pq, kq = self._in(q, self.dof)
        pd, kd = self._in(dq, self.dof)
        self._rc(self.lib.sai2b_set_state(self.h, pq, pd, self._dev(q, dq)))

    def set_mft_goals(self, task, pos=None, rot=None, v=None, w=None, a=None, alpha=None):
        objs = (pos, rot, v, w, a, alpha)
        ins = [self._in(o, r) for o, r in zip(objs, (3, 9, 3, 3, 3, 3))]
        self._rc(self.lib.sai2b_set_mft_goals(self.h, task, *[p for p, _ in ins], self._dev(*objs)))

    def set_mft_goal_wrench(self, task, f=None, m=None):
        ins = [self._in(f, 3), self._in(m, 3)]
        self._rc(self.lib.sai2b_set_mft_goal_wrench(self.h, task, ins[0][0], ins[1][0], self._dev(f, m)))

    def set_mft_sensed_wrench(self, task, f=None, m=None):
        ins = [self._in(f, 3), self._in(m, 3)]
        self._rc(self.lib.sai2b_set_mft_sensed_wrench(self.h, task, ins[0][0], ins[1][0], self._dev(f, m)))

    def set_jt_goals(self, task, q=None, dq=None, ddq=None):
        if not (0 <= task < len(self.tasks)) or self.tasks[task].type != _abi.JOINT_TASK:
            raise ValueError("sai2b_set_jt_goals: task is not a JointTask")
        k0 = self.tasks[task].task_dof
        ins = [self._in(o, k0) for o in (q, dq, ddq)]
        self._rc(self.lib.sai2b_set_jt_goals(self.h, task, *[p for p, _ in ins], self._dev(q, dq, ddq)))

    # -- per-robot payloads (sai2b.h "per-robot payloads")
    @staticmethod
    def _payload_target(target):
        try:
            return _abi.PAYLOAD_TARGETS[target] if isinstance(target, str) else int(target)
        except KeyError:
            raise ValueError("target must be 'controller', 'plant' or 'both'") from None

    def set_link_payload(self, link, mass, com=None, inertia=None, target="both"):
        """one rigid body per robot on moving link `link`: mass [B], com [3][B] in the link frame (None: zeros), inertia
        [6][B] about the body's COM (ixx iyy izz ixy ixz iyz; None: point mass); numpy arrays or torch CUDA tensors.
        target: 'controller' (what M, g and the torques are computed with), 'plant' (what sim_step integrates) or 'both'"""
        if mass is not None and not hasattr(mass, "data_ptr"):
            mass = np.ascontiguousarray(mass, dtype=np.float64).reshape(1, -1)
        elif mass is not None and mass.dim() == 1:
            mass = mass.view(1, -1)
        ins = [self._in(o, r) for o, r in zip((mass, com, inertia), (1, 3, 6))]
        self._rc(self.lib.sai2b_set_link_payload(self.h, self._payload_target(target), int(link), *[p for p, _ in ins],
                                                 self._dev(mass, com, inertia)))

    def clear_link_payload(self, target="both"):
        self._rc(self.lib.sai2b_clear_link_payload(self.h, self._payload_target(target)))

    def get_link_payload(self, target="controller"):
        """-> (link, mass [B], com [3][B], inertia [6][B]) of one target; link -1 and zeros when it has no payload"""
        link = C.c_int()
        m, c, i = np.empty(self.B), np.empty((3, self.B)), np.empty((6, self.B))
        self._rc(self.lib.sai2b_get_link_payload(self.h, self._payload_target(target), C.byref(link),
                                                 *[C.c_void_p(x.ctypes.data) for x in (m, c, i)]))
        return link.value, m, c, i

    # -- contact in the simulated plant (sai2b.h "contact in the simulated plant")
    def contact_config(self, link, points=None, sensor_task=-1, friction_velocity_eps=1e-3):
        """-> ContactConfig: `points` [n][3] in the frame of moving link `link` (None: the link origin), 1 <= n <= 4"""
        pts = np.zeros((1, 3)) if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cfg = _abi.ContactConfig()
        rc = self.lib.sai2b_default_contact(C.byref(cfg), int(link), int(pts.shape[0]), pts.ctypes.data_as(C.POINTER(C.c_double)))
        if rc:
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        cfg.sensor_task = int(sensor_task)
        cfg.friction_velocity_eps = float(friction_velocity_eps)
        return cfg

    def set_contact(self, link, points, plane_point, plane_normal, stiffness, damping=None, friction=None, sensor_task=-1,
                    friction_velocity_eps=1e-3):
        """every robot's own surface for sim_step: contact points [n][3] fixed to `link` (or a ContactConfig as `link`, then
        `points` is ignored), per robot plane_point [3][B], unit plane_normal [3][B] (out of the surface), stiffness [B] (N/m),
        damping [B] (s/m, None: 0), friction [B] (None: 0); numpy arrays or torch CUDA tensors. sensor_task: the MotionForceTask
        whose sensed rows the simulated force / moment sensor writes after every step (-1: none)"""
        if isinstance(link, _abi.ContactConfig):
            if points is not None or sensor_task != -1 or friction_velocity_eps != 1e-3:
                raise ValueError("set_contact: a ContactConfig carries its own points, sensor_task and friction_velocity_eps")
            cfg = link
        else:
            cfg = self.contact_config(link, points, sensor_task, friction_velocity_eps)

        def row(a):
            if a is None or hasattr(a, "data_ptr"):
                return a if a is None or a.dim() == 2 else a.view(1, -1)
            return np.ascontiguousarray(a, dtype=np.float64).reshape(1, -1)

        k, d, mu = row(stiffness), row(damping), row(friction)
        ins = [self._in(o, r) for o, r in zip((plane_point, plane_normal, k, d, mu), (3, 3, 1, 1, 1))]
        self._rc(self.lib.sai2b_set_contact(self.h, C.byref(cfg), *[p for p, _ in ins], self._dev(plane_point, plane_normal, k, d, mu)))

    def clear_contact(self):
        self._rc(self.lib.sai2b_clear_contact(self.h))

    def get_contact(self):
        """-> (ContactConfig, rows [9][B]); n_points 0 and zeros when the plant has no contact"""
        cfg, rows = _abi.ContactConfig(), np.empty((9, self.B))
        self._rc(self.lib.sai2b_get_contact(self.h, C.byref(cfg), C.c_void_p(rows.ctypes.data)))
        return cfg, rows

    def get_contact_state(self):
        """what the last sim_step left: dict depth [4][B], normal_force [4][B], wrench_world [6][B], robots_in_contact"""
        n = C.c_int()
        out = [np.empty((r, self.B)) for r in (4, 4, 6)]
        self._rc(self.lib.sai2b_get_contact_state(self.h, *[C.c_void_p(x.ctypes.data) for x in out], C.byref(n)))
        return dict(depth=out[0], normal_force=out[1], wrench_world=out[2], robots_in_contact=n.value)

    def robots_in_contact(self):
        n = C.c_int()
        self._rc(self.lib.sai2b_get_contact_state(self.h, None, None, None, C.byref(n)))
        return n.value

    # -- joint dynamics of the simulated plant (sai2b.h "joint dynamics of the simulated plant")
    def joint_dynamics_config(self, stop_stiffness=0.0, stop_damping=0.0, friction_velocity_eps=1e-2):
        """-> JointDynamicsConfig: each a scalar or [dof] (batch-uniform, per joint)"""
        cfg = _abi.JointDynamicsConfig()
        if self.lib.sai2b_default_joint_dynamics(C.byref(cfg), self.dof):
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        for name, v in (("stop_stiffness", stop_stiffness), ("stop_damping", stop_damping), ("friction_velocity_eps", friction_velocity_eps)):
            a = np.asarray(v, dtype=np.float64)
            if a.ndim > 1 or (a.ndim == 1 and a.shape != (self.dof,)):
                raise ValueError(f"{name}: expected a scalar or {self.dof} values")
            getattr(cfg, name)[: self.dof] = [float(x) for x in np.broadcast_to(a, (self.dof,))]
        msg = C.create_string_buffer(256)
        if self.lib.sai2b_validate_joint_dynamics(C.byref(cfg), self.dof, msg, 256):
            raise ValueError(msg.value.decode())
        return cfg

    def _joint_row(self, a, name):
        """a scalar, [dof] or [dof][B] -> [dof][B] float64; a torch CUDA tensor [dof][B] passes as it is"""
        if a is None or hasattr(a, "data_ptr"):
            return a
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1 and a.shape == (self.dof,):
            a = a[:, None]
        elif a.ndim not in (0, 2) or (a.ndim == 2 and a.shape != (self.dof, self.B)):
            raise ValueError(f"{name}: expected a scalar, {self.dof} values or an array of shape ({self.dof}, {self.B})")
        return np.ascontiguousarray(np.broadcast_to(a, (self.dof, self.B)))

    def set_joint_dynamics(self, armature=None, damping=None, friction=None, torque_limit=None, q_lower=None, q_upper=None,
                           stop_stiffness=0.0, stop_damping=0.0, friction_velocity_eps=1e-2, limits=None):
        """every robot's own joints for sim_step: armature, damping, Coulomb friction level, torque limit and joint limits, each
        a scalar, [dof] or [dof][B] (numpy; broadcast) or a torch CUDA tensor [dof][B]; None: that effect off.
        torque_limit="model" takes the effort limits and limits="model" the q_lower / q_upper of the context's model.
        stop_stiffness, stop_damping, friction_velocity_eps: scalars or [dof], batch-uniform; or a
        JointDynamicsConfig as `stop_stiffness`"""
        if isinstance(torque_limit, str) or isinstance(limits, str):
            model = self.model
            if isinstance(torque_limit, str):
                if torque_limit != "model":
                    raise ValueError("torque_limit must be an array or 'model'")
                torque_limit = np.array(model.effort[: self.dof])
            if isinstance(limits, str):
                if limits != "model" or q_lower is not None or q_upper is not None:
                    raise ValueError("limits must be 'model', without q_lower / q_upper")
                q_lower, q_upper = np.array(model.q_lower[: self.dof]), np.array(model.q_upper[: self.dof])
        elif limits is not None:
            raise ValueError("limits must be 'model' or None")
        if isinstance(stop_stiffness, _abi.JointDynamicsConfig):
            cfg = stop_stiffness
        else:
            cfg = self.joint_dynamics_config(stop_stiffness, stop_damping, friction_velocity_eps)
        objs = [self._joint_row(o, n) for o, n in zip((armature, damping, friction, torque_limit, q_lower, q_upper), _abi.JOINT_DYNAMICS_ROWS)]
        ins = [self._in(o, self.dof) for o in objs]
        self._rc(self.lib.sai2b_set_joint_dynamics(self.h, C.byref(cfg), *[p for p, _ in ins], self._dev(*objs)))

    def clear_joint_dynamics(self):
        self._rc(self.lib.sai2b_clear_joint_dynamics(self.h))

    def get_joint_dynamics(self):
        """-> (JointDynamicsConfig, rows [6][dof][B]); the defaults and the neutral rows when the plant has no joint dynamics"""
        cfg, rows = _abi.JointDynamicsConfig(), np.empty((6, self.dof, self.B))
        self._rc(self.lib.sai2b_get_joint_dynamics(self.h, C.byref(cfg), C.c_void_p(rows.ctypes.data)))
        return cfg, rows

    def get_joint_dynamics_state(self):
        """what the last sim_step left: dict applied_torque, stop_torque, dissipative_torque [dof][B], robots_saturated,
        robots_at_stop"""
        ns, na = C.c_int(), C.c_int()
        out = [np.empty((self.dof, self.B)) for _ in range(3)]
        self._rc(self.lib.sai2b_get_joint_dynamics_state(self.h, *[C.c_void_p(x.ctypes.data) for x in out], C.byref(ns), C.byref(na)))
        return dict(applied_torque=out[0], stop_torque=out[1], dissipative_torque=out[2], robots_saturated=ns.value,
                    robots_at_stop=na.value)

    def robots_saturated(self):
        n = C.c_int()
        self._rc(self.lib.sai2b_get_joint_dynamics_state(self.h, None, None, None, C.byref(n), None))
        return n.value

    def robots_at_stop(self):
        n = C.c_int()
        self._rc(self.lib.sai2b_get_joint_dynamics_state(self.h, None, None, None, None, C.byref(n)))
        return n.value

    # -- external wrench on a link of the simulated plant (sai2b.h "external wrench on a link of the simulated plant")
    def external_wrench_config(self, link, point=(0.0, 0.0, 0.0), frame="world", sensor_task=-1):
        """-> ExternalWrenchConfig: application `point` in the frame of moving link `link`; frame 'world' or 'link'"""
        cfg = _abi.ExternalWrenchConfig()
        if self.lib.sai2b_default_external_wrench(C.byref(cfg), int(link)):
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        try:
            cfg.frame = _abi.WRENCH_FRAMES[frame] if isinstance(frame, str) else int(frame)
        except KeyError:
            raise ValueError("frame must be 'world' or 'link'") from None
        p = np.asarray(point, dtype=np.float64)
        if p.shape != (3,):
            raise ValueError("point: expected 3 values")
        cfg.point[:] = [float(x) for x in p]
        cfg.sensor_task = int(sensor_task)
        msg = C.create_string_buffer(256)
        tasks = (_abi.TaskConfig * len(self.tasks))(*self.tasks)
        if self.lib.sai2b_validate_external_wrench(C.byref(cfg), tasks, len(self.tasks), self.dof, msg, 256):
            raise ValueError(msg.value.decode())
        return cfg

    def set_external_wrench(self, link, force, moment=None, steps=None, point=(0.0, 0.0, 0.0), frame="world", sensor_task=-1):
        """every robot's own push for sim_step: force [3][B] (N) and moment [3][B] (a pure couple, N m; None: 0) on moving link
        `link` at `point` (link frame), world components or, with frame='link', components that turn with the link; steps [B]:
        the robot's remaining pushed periods (> 0 counted down by every sim_step, < 0 until changed, 0 off; None: -1). numpy
        arrays ([3] broadcasts over the batch, a scalar `steps` too) or torch CUDA tensors [3][B] / [B]. sensor_task: the
        MotionForceTask whose sensed rows read the wrench after every step (-1: none). An ExternalWrenchConfig as `link`
        carries its own point, frame and sensor_task"""
        if isinstance(link, _abi.ExternalWrenchConfig):
            if tuple(point) != (0.0, 0.0, 0.0) or frame != "world" or sensor_task != -1:
                raise ValueError("set_external_wrench: an ExternalWrenchConfig carries its own point, frame and sensor_task")
            cfg = link
        else:
            cfg = self.external_wrench_config(link, point, frame, sensor_task)

        def rows3(a, name):
            if a is None or hasattr(a, "data_ptr"):
                return a
            a = np.asarray(a, dtype=np.float64)
            if a.shape == (3,):
                a = a[:, None]
            elif a.shape != (3, self.B):
                raise ValueError(f"{name}: expected 3 values or an array of shape (3, {self.B})")
            return np.ascontiguousarray(np.broadcast_to(a, (3, self.B)))

        f, m = rows3(force, "force"), rows3(moment, "moment")
        if steps is not None and hasattr(steps, "data_ptr"):
            s = steps if steps.dim() == 2 else steps.view(1, -1)
        elif steps is not None:
            s = np.asarray(steps, dtype=np.float64)
            if s.ndim > 1 and s.shape != (1, self.B) or s.ndim == 1 and s.shape != (self.B,):
                raise ValueError(f"steps: expected a scalar or {self.B} values")
            s = np.ascontiguousarray(np.broadcast_to(s.reshape(1, -1) if s.ndim else s, (1, self.B)))
        else:
            s = None
        ins = [self._in(o, r) for o, r in zip((f, m, s), (3, 3, 1))]
        self._rc(self.lib.sai2b_set_external_wrench(self.h, C.byref(cfg), *[p for p, _ in ins], self._dev(f, m, s)))

    def clear_external_wrench(self):
        self._rc(self.lib.sai2b_clear_external_wrench(self.h))

    def get_external_wrench(self):
        """-> (ExternalWrenchConfig, rows [7][B]: force 3, moment 3, steps); link -1 and zeros when the plant has no wrench"""
        cfg, rows = _abi.ExternalWrenchConfig(), np.empty((7, self.B))
        self._rc(self.lib.sai2b_get_external_wrench(self.h, C.byref(cfg), C.c_void_p(rows.ctypes.data)))
        return cfg, rows

    def get_external_wrench_state(self):
        """what the last sim_step left: dict wrench_world [6][B] (F_w, M_w about the point), torque [dof][B], robots_pushed"""
        n = C.c_int()
        w, t = np.empty((6, self.B)), np.empty((self.dof, self.B))
        self._rc(self.lib.sai2b_get_external_wrench_state(self.h, C.c_void_p(w.ctypes.data), C.c_void_p(t.ctypes.data), C.byref(n)))
        return dict(wrench_world=w, torque=t, robots_pushed=n.value)

    def robots_pushed(self):
        n = C.c_int()
        self._rc(self.lib.sai2b_get_external_wrench_state(self.h, None, None, C.byref(n)))
        return n.value

    # -- actuator and force-sensor models (sai2b.h "actuator and force-sensor models")
    def hardware_config(self, max_delay=0, sensor_task=-1, seed=0, first_robot=0):
        """-> HardwareConfig, validated against this controller's tasks"""
        cfg = _abi.HardwareConfig()
        if self.lib.sai2b_default_hardware(C.byref(cfg)):
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        cfg.max_delay, cfg.sensor_task = int(max_delay), int(sensor_task)
        cfg.seed, cfg.first_robot = int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_robot) & 0xFFFFFFFF
        msg = C.create_string_buffer(256)
        tasks = (_abi.TaskConfig * len(self.tasks))(*self.tasks)
        if self.lib.sai2b_validate_hardware(C.byref(cfg), tasks, len(self.tasks), self.dof, msg, 256):
            raise ValueError(msg.value.decode())
        return cfg

    def hardware_rows(self, delay=0, lag=1.0, gain=1.0, noise=0.0, bias=0.0, sensor_noise=0.0, sensor_filter=1.0):
        """-> (actuator_rows [1 + 3 dof][B], sensor_rows [13][B]) as numpy arrays: delay [B] in periods; lag, gain and noise
        [dof][B] (the lag coefficient alpha, the gain k, the noise deviation sigma); bias and sensor_noise [6][B];
        sensor_filter [B]. A scalar, or a [dof] / [6] column, is the same for every robot. The defaults are the ideal path."""
        n, B = self.dof, self.B

        def block(a, rows, name):
            a = np.asarray(a, dtype=np.float64)
            if a.ndim == 1 and a.shape[0] == rows and rows != B:
                a = a[:, None]
            try:
                return np.broadcast_to(a, (rows, B))
            except ValueError:
                raise ValueError(f"{name}: expected a scalar, {rows} values or an array of shape ({rows}, {B})") from None

        act = np.empty((1 + 3 * n, B))
        act[0] = np.broadcast_to(np.asarray(delay, dtype=np.float64), (B,))
        act[1 : 1 + n], act[1 + n : 1 + 2 * n], act[1 + 2 * n :] = block(lag, n, "lag"), block(gain, n, "gain"), block(noise, n, "noise")
        sen = np.empty((_abi.HARDWARE_SENSOR_ROWS, B))
        sen[0:6], sen[6:12] = block(bias, 6, "bias"), block(sensor_noise, 6, "sensor_noise")
        sen[12] = np.broadcast_to(np.asarray(sensor_filter, dtype=np.float64), (B,))
        return act, sen

    def set_hardware(self, actuator_rows=None, sensor_rows=None, max_delay=0, sensor_task=-1, seed=0, first_robot=0, config=None):
        """the signal path of every robot for sim_step: actuator_rows [1 + 3 dof][B] (delay, lag coefficient, gain, noise
        deviation) and sensor_rows [13][B] (bias 6, noise deviation 6, filter coefficient), numpy or torch CUDA, None = ideal
        (hardware_rows() builds them); max_delay: depth D of the torque history; sensor_task: the MotionForceTask whose sensed
        rows become the measured wrench (-1: none); seed, first_robot: the random generator's key and the global index of this
        controller's robot 0. A HardwareConfig as `config` carries max_delay, sensor_task, seed and first_robot. Restarts every
        robot's period and episode counters."""
        cfg = config if config is not None else self.hardware_config(max_delay, sensor_task, seed, first_robot)
        rows = (1 + 3 * self.dof, _abi.HARDWARE_SENSOR_ROWS)
        objs = []
        for a, r, name in zip((actuator_rows, sensor_rows), rows, ("actuator_rows", "sensor_rows")):
            if a is not None and not hasattr(a, "data_ptr"):
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (r, self.B):
                    raise ValueError(f"{name}: expected an array of shape ({r}, {self.B})")
            objs.append(a)
        ins = [self._in(o, r) for o, r in zip(objs, rows)]
        self._rc(self.lib.sai2b_set_hardware(self.h, C.byref(cfg), ins[0][0], ins[1][0], self._dev(*objs)))

    def clear_hardware(self):
        self._rc(self.lib.sai2b_clear_hardware(self.h))

    def get_hardware(self):
        """-> (HardwareConfig, actuator_rows [1 + 3 dof][B], sensor_rows [13][B]); the default configuration and the ideal rows
        when no hardware is set"""
        cfg = _abi.HardwareConfig()
        act, sen = np.empty((1 + 3 * self.dof, self.B)), np.empty((_abi.HARDWARE_SENSOR_ROWS, self.B))
        self._rc(self.lib.sai2b_get_hardware(self.h, C.byref(cfg), C.c_void_p(act.ctypes.data), C.c_void_p(sen.ctypes.data)))
        return cfg, act, sen

    def get_hardware_state(self):
        """what the last sim_step left: dict applied_torque [dof][B], period [B], episode [B] (int32)"""
        a = np.empty((self.dof, self.B))
        n, e = np.empty(self.B, dtype=np.int32), np.empty(self.B, dtype=np.int32)
        self._rc(self.lib.sai2b_get_hardware_state(self.h, C.c_void_p(a.ctypes.data), C.c_void_p(n.ctypes.data), C.c_void_p(e.ctypes.data)))
        return dict(applied_torque=a, period=n, episode=e)

    # -- joint sensors (sai2b.h "joint sensors")
    def joint_sensor_config(self, max_delay=0, velocity_mode="tachometer", seed=0, first_robot=0):
        """-> JointSensorConfig, validated. velocity_mode: 'tachometer' or 'finite_difference' (or 0 / 1)"""
        cfg = _abi.JointSensorConfig()
        if self.lib.sai2b_default_joint_sensor(C.byref(cfg)):
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        if isinstance(velocity_mode, str):
            if velocity_mode not in _abi.JOINT_SENSOR_VELOCITY_MODES:
                raise ValueError("velocity_mode must be 'tachometer' or 'finite_difference'")
            velocity_mode = _abi.JOINT_SENSOR_VELOCITY_MODES[velocity_mode]
        cfg.max_delay, cfg.velocity_mode = int(max_delay), int(velocity_mode)
        cfg.seed, cfg.first_robot = int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_robot) & 0xFFFFFFFF
        msg = C.create_string_buffer(256)
        if self.lib.sai2b_validate_joint_sensor(C.byref(cfg), self.dof, msg, 256):
            raise ValueError(msg.value.decode())
        return cfg

    def joint_sensor_rows(self, delay=0, offset=0.0, noise=0.0, quantum=0.0, velocity_noise=0.0, velocity_alpha=1.0):
        """-> rows [1 + 5 dof][B]: delay [B] in periods; offset, noise (position noise deviation), quantum, velocity_noise and
        velocity_alpha (the velocity filter's coefficient) [dof][B]. A scalar, or a [dof] column, is the same for every robot.
        numpy in, numpy out; when any argument is a torch CUDA tensor the rows are a CUDA tensor on this controller's device.
        The defaults are the ideal sensor."""
        n, B = self.dof, self.B
        args = (delay, offset, noise, quantum, velocity_noise, velocity_alpha)
        if any(hasattr(a, "data_ptr") for a in args):
            import torch

            dev = f"cuda:{self._device}"
            out = torch.empty((1 + 5 * n, B), dtype=torch.float64, device=dev)

            def block(a, rows, name):
                a = torch.as_tensor(a, dtype=torch.float64, device=dev)
                if a.dim() == 1 and a.shape[0] == rows and rows != B:
                    a = a[:, None]
                try:
                    return torch.broadcast_to(a, (rows, B))
                except RuntimeError:
                    raise ValueError(f"{name}: expected a scalar, {rows} values or an array of shape ({rows}, {B})") from None

        else:
            out = np.empty((1 + 5 * n, B))

            def block(a, rows, name):
                a = np.asarray(a, dtype=np.float64)
                if a.ndim == 1 and a.shape[0] == rows and rows != B:
                    a = a[:, None]
                try:
                    return np.broadcast_to(a, (rows, B))
                except ValueError:
                    raise ValueError(f"{name}: expected a scalar, {rows} values or an array of shape ({rows}, {B})") from None

        out[0:1] = block(delay, 1, "delay")
        for k, (a, name) in enumerate(zip(args[1:], ("offset", "noise", "quantum", "velocity_noise", "velocity_alpha"))):
            out[1 + k * n : 1 + (k + 1) * n] = block(a, n, name)
        return out

    def set_joint_sensor(self, rows=None, *, max_delay=0, velocity_mode="tachometer", seed=0, first_robot=0, config=None):
        """the controller's view of every robot's joint state: rows [1 + 5 dof][B] (joint_sensor_rows() builds them), numpy or
        torch CUDA, None = ideal; max_delay: depth D of the reading history; velocity_mode: 'tachometer' or
        'finite_difference'; seed, first_robot: the random generator's key and the global index of this controller's robot 0.
        A JointSensorConfig as `config` carries the four. From here on tick, observe and apply_action read measured_state(),
        sim_step, set_state, get_state and the resets the truth. Seeds every robot's measurement and zeroes its clocks."""
        cfg = config if config is not None else self.joint_sensor_config(max_delay, velocity_mode, seed, first_robot)
        r = 1 + 5 * self.dof
        if rows is not None and not hasattr(rows, "data_ptr"):
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            if rows.shape != (r, self.B):
                raise ValueError(f"rows: expected an array of shape ({r}, {self.B})")
        ptr, _keep = self._in(rows, r)
        self._rc(self.lib.sai2b_set_joint_sensor(self.h, C.byref(cfg), ptr, self._dev(rows)))

    def clear_joint_sensor(self):
        self._rc(self.lib.sai2b_clear_joint_sensor(self.h))

    def joint_sensor(self):
        """-> (JointSensorConfig, rows [1 + 5 dof][B]); the default configuration and the ideal rows when none is set"""
        cfg, rows = _abi.JointSensorConfig(), np.empty((1 + 5 * self.dof, self.B))
        self._rc(self.lib.sai2b_get_joint_sensor(self.h, C.byref(cfg), C.c_void_p(rows.ctypes.data)))
        return cfg, rows

    def joint_sensor_state(self):
        """-> dict clock [B]: the index of the next reading, episode [B] (int32); zeros without a joint sensor"""
        c, e = np.empty(self.B, dtype=np.int32), np.empty(self.B, dtype=np.int32)
        self._rc(self.lib.sai2b_get_joint_sensor_state(self.h, C.c_void_p(c.ctypes.data), C.c_void_p(e.ctypes.data)))
        return dict(clock=c, episode=e)

    def get_measured_state(self):
        """-> (q, dq) [dof][B] as numpy arrays: the measured pair; the truth without a joint sensor"""
        q, dq = np.empty((self.dof, self.B)), np.empty((self.dof, self.B))
        self._rc(self.lib.sai2b_get_measured_state(self.h, C.c_void_p(q.ctypes.data), C.c_void_p(dq.ctypes.data)))
        return q, dq

    def measured_state(self):
        """the measured q and dq as torch views of the two device buffers (no copy), [dof][B] float64. Order reads with
        stream()."""
        import torch

        pq, pd = self.device_buffer(_abi.BUF_Q_MEASURED), self.device_buffer(_abi.BUF_DQ_MEASURED)
        if not pq or not pd:
            raise ValueError("measured_state: no joint sensor is set (sai2b_set_joint_sensor)")

        def view(ptr):
            class _Buf:
                __cuda_array_interface__ = dict(shape=(self.dof, self.B), typestr="<f8", data=(int(ptr), False), version=2)

            return torch.as_tensor(_Buf(), device=f"cuda:{self._device}")

        return view(pq), view(pd)

    # -- collision proximity and episodes ended from outside (sai2b.h "collision proximity")
    def collision_config(self, *args, **kwargs):
        """collision_config() of this module for this controller's robot"""
        return collision_config(self.dof, *args, **kwargs)

    def collision_env_rows(self, cfg, planes=(), obstacles=()):
        """-> rows [6 P + 4 O][B] (numpy): planes: per plane (point [3] or [3][B], unit normal [3] or [3][B]); obstacles: per obstacle
        (centre [3] or [3][B], radius scalar or [B]); one not given is absent (NaN)"""
        P, O, B = cfg.n_planes, cfg.n_obstacles, self.B
        rows = np.full((6 * P + 4 * O, B), np.nan)
        if len(planes) > P or len(obstacles) > O:
            raise ValueError("collision: more planes or obstacles than the configuration has")
        col = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(3, -1), (3, B))
        for k, (p0, nrm) in enumerate(planes):
            rows[6 * k : 6 * k + 3], rows[6 * k + 3 : 6 * k + 6] = col(p0), col(nrm)
        for k, (c, r) in enumerate(obstacles):
            rows[6 * P + 4 * k : 6 * P + 4 * k + 3], rows[6 * P + 4 * k + 3] = col(c), np.broadcast_to(np.asarray(r, dtype=np.float64), (B,))
        return rows

    def set_collision(self, cfg=None, rows=None, **kwargs):
        """the arm's proximity sensor: a CollisionConfig (or the arguments of collision_config) and the per-robot environment rows
        [6 P + 4 O][B], numpy (validated) or torch CUDA (copied as they are); None: every plane and obstacle absent until a
        producer writes device_buffer(_abi.BUF_COLLISION). Nothing else in the controller changes."""
        if cfg is None:
            cfg = self.collision_config(**kwargs)
        elif kwargs:
            raise ValueError("set_collision: a CollisionConfig or keyword arguments, not both")
        r = 6 * cfg.n_planes + 4 * cfg.n_obstacles
        if rows is not None and r == 0:
            raise ValueError("rows: the configuration has no plane and no obstacle")
        if rows is not None and not hasattr(rows, "data_ptr"):
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            if rows.shape != (r, self.B):
                raise ValueError(f"rows: expected an array of shape ({r}, {self.B})")
        ptr, _keep = self._in(rows, r)
        self._rc(self.lib.sai2b_set_collision(self.h, C.byref(cfg), ptr, self._dev(rows)))

    def clear_collision(self):
        self._rc(self.lib.sai2b_clear_collision(self.h))

    def get_collision(self):
        """-> (CollisionConfig, rows [6 P + 4 O][B])"""
        cfg = _abi.CollisionConfig()
        self._rc(self.lib.sai2b_get_collision(self.h, C.byref(cfg), None))
        rows = np.empty((6 * cfg.n_planes + 4 * cfg.n_obstacles, self.B))
        if rows.shape[0]:
            self._rc(self.lib.sai2b_get_collision(self.h, None, C.c_void_p(rows.ctypes.data)))
        return cfg, rows

    def collision_env(self):
        """the per-robot environment rows as a torch view of the device buffer (no copy), [6 P + 4 O][B] float64: a torch op may
        move an obstacle every period; the next collision_query reads what it wrote. Order writes with stream()."""
        import torch

        ptr = self.device_buffer(_abi.BUF_COLLISION)
        if not ptr:
            raise ValueError("collision_env: no collision geometry with a plane or an obstacle is set (sai2b_set_collision)")
        cfg = _abi.CollisionConfig()
        self._rc(self.lib.sai2b_get_collision(self.h, C.byref(cfg), None))
        shape = (6 * cfg.n_planes + 4 * cfg.n_obstacles, self.B)

        class _Buf:
            __cuda_array_interface__ = dict(shape=shape, typestr="<f8", data=(int(ptr), False), version=2)

        return torch.as_tensor(_Buf(), device=f"cuda:{self._device}")

    def collision_rows(self):
        """rows of the configured output; -1 without a configuration"""
        return self.lib.sai2b_collision_rows(self.h)

    def collision_layout(self):
        """dict name -> slice of rows of collision_query()'s output: 'distance', 'index', 'normal', 'gradient', 'centres' and, for
        the first four, 'distance_plane', 'distance_obstacle', 'distance_self', ...; only what the configuration stores"""
        first, n = C.c_int(), C.c_int()
        out = {}
        for name, flag in _abi.COL_BLOCKS.items():
            self._rc(self.lib.sai2b_collision_layout(self.h, flag, -1, C.byref(first), C.byref(n)))
            if not n.value:
                continue
            out[name] = slice(first.value, first.value + n.value)
            if flag != _abi.COL_CENTRES:
                for c, cat in enumerate(_abi.COL_CATEGORIES):
                    self._rc(self.lib.sai2b_collision_layout(self.h, flag, c, C.byref(first), C.byref(n)))
                    out[f"{name}_{cat}"] = slice(first.value, first.value + n.value)
        return out

    def collision_query(self, out=None, flags=None):
        """one launch -> (rows [collision_rows()][B] float64, flags [B] uint8 with the _abi.COL_FLAGS bits). out / flags: numpy
        arrays or torch CUDA tensors to fill (both of one kind; a torch pair never leaves the device and nothing synchronises),
        None: a new numpy array, False: not wanted (None is returned in its place)"""
        rows = self.collision_rows()
        if rows < 0:
            raise ValueError("sai2b_collision_query: no collision geometry is configured (sai2b_set_collision)")
        given = [o for o in (out, flags) if o is not None and o is not False]
        dev = self._dev(*given)
        if dev and (out is None or flags is None):
            raise ValueError("collision_query: with a device tensor pass the other argument as a tensor too, or False")
        if out is None:
            out = np.empty((rows, self.B))
        if flags is None:
            flags = np.zeros(self.B, dtype=np.uint8)
        po = pf = None
        if out is not False:
            if hasattr(out, "data_ptr"):
                po, _ = self._in(out, rows)
            else:
                if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (rows, self.B)):
                    raise ValueError(f"out must be a C-contiguous float64 array of shape ({rows}, {self.B})")
                po = C.c_void_p(out.ctypes.data)
        if flags is not False:
            if hasattr(flags, "data_ptr"):
                if str(flags.dtype) != "torch.uint8":
                    raise ValueError("flags must be a uint8 tensor (it receives the flag bits)")
                pf, _ = self._mask(flags)
            else:
                if not (isinstance(flags, np.ndarray) and flags.dtype == np.uint8 and flags.flags.c_contiguous and flags.shape == (self.B,)):
                    raise ValueError(f"flags must be a C-contiguous uint8 array of shape ({self.B},)")
                pf = C.c_void_p(flags.ctypes.data)
        self._rc(self.lib.sai2b_collision_query(self.h, po, pf, dev))
        return (None if out is False else out), (None if flags is False else flags)

    def collision_counts(self):
        """of the last collision_query(): dict 'plane', 'obstacle', 'self', 'nonfinite' -> robots with that bit, 'any' -> robots
        with a non-zero byte"""
        c = (C.c_int * 5)()
        self._rc(self.lib.sai2b_get_collision_counts(self.h, c))
        return dict(zip(list(_abi.COL_FLAGS) + ["any"], list(c)))

    def end_episodes(self, done, extra, bit=_abi.DONE_COLLISION):
        """one launch: the episodes of the robots with extra != 0 that are not done yet are closed as observe_reward closes one,
        then their done bytes gain `bit` (64 or 128). done: [B] uint8, updated in place; extra: [B] uint8 or bool; both numpy or
        both torch CUDA (then nothing synchronises). -> done"""
        if int(bit) not in (64, 128):
            raise ValueError("sai2b_end_episodes: bit must be 64 or 128")
        dev = self._dev(done, extra)
        if dev:
            if str(done.dtype) != "torch.uint8":
                raise ValueError("done must be a uint8 tensor (it receives the bit)")
        elif not (isinstance(done, np.ndarray) and done.dtype == np.uint8 and done.flags.c_contiguous and done.shape == (self.B,)):
            raise ValueError(f"done must be a C-contiguous uint8 array of shape ({self.B},)")
        pd, _kd = self._mask(done)
        pe, _ke = self._mask(extra)
        self._rc(self.lib.sai2b_end_episodes(self.h, pd, pe, int(bit), dev))
        return done

    def end_episode_count(self):
        """robots whose episode the last end_episodes() closed"""
        c = C.c_int()
        self._rc(self.lib.sai2b_get_end_episode_count(self.h, C.byref(c)))
        return c.value

    # -- whole-arm contact of the simulated plant (sai2b.h "whole-arm contact")
    def body_contact_config(self, *args, **kwargs):
        """body_contact_config() of this module for this controller's robot"""
        return body_contact_config(self.dof, *args, **kwargs)

    def set_body_contact(self, stiffness, damping=0.0, friction=0.0, cfg=None, **kwargs):
        """the collision configuration's spheres as a physical body for sim_step: stiffness k (N/m), damping d (s/m) and friction
        mu per robot, scalars or [B] numpy arrays (validated: finite and >= 0), or `stiffness` alone as the whole [3][B] rows,
        numpy or a torch CUDA tensor (copied as it is). cfg: a BodyContactConfig, or the keyword arguments of
        body_contact_config. Needs set_collision first; the environment rows are read live at every step."""
        if cfg is None:
            cfg = self.body_contact_config(**kwargs)
        elif kwargs:
            raise ValueError("set_body_contact: a BodyContactConfig or keyword arguments, not both")
        if hasattr(stiffness, "data_ptr"):
            rows = stiffness
        else:
            k = np.asarray(stiffness, dtype=np.float64)
            if k.shape == (3, self.B):
                rows = np.ascontiguousarray(k)
            else:
                try:
                    rows = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(a, dtype=np.float64), (self.B,)) for a in (k, damping, friction)]))
                except ValueError:
                    raise ValueError(f"stiffness, damping, friction: expected scalars or {self.B} values each") from None
        ptr, _keep = self._in(rows, 3)
        self._rc(self.lib.sai2b_set_body_contact(self.h, C.byref(cfg), ptr, self._dev(rows)))

    def clear_body_contact(self):
        self._rc(self.lib.sai2b_clear_body_contact(self.h))

    def get_body_contact(self):
        """-> (BodyContactConfig, rows [3][B]: stiffness, damping, friction); categories 0 and zeros without one"""
        cfg, rows = _abi.BodyContactConfig(), np.empty((3, self.B))
        self._rc(self.lib.sai2b_get_body_contact(self.h, C.byref(cfg), C.c_void_p(rows.ctypes.data)))
        return cfg, rows

    def get_body_contact_state(self):
        """what the last sim_step left: dict depth [3][B] (deepest penetration of plane, obstacle, self), index [3][B] (its
        witness, -1: none), normal_force [3][B] (sum of f_n), torque [dof][B] (tb), status (all rows, [9 + dof][B]), counts
        (dict 'plane', 'obstacle', 'self', 'any' -> robots with some f_n > 0)"""
        st, c = np.empty((9 + self.dof, self.B)), (C.c_int * 4)()
        self._rc(self.lib.sai2b_get_body_contact_state(self.h, C.c_void_p(st.ctypes.data), c))
        return dict(depth=st[0:3], index=st[3:6].astype(np.int64), normal_force=st[6:9], torque=st[9:], status=st,
                    counts=dict(zip(_abi.BODY_CONTACT_COUNTS, list(c))))

    def robots_touching(self):
        """robots with some f_n > 0 after the last sim_step"""
        c = (C.c_int * 4)()
        self._rc(self.lib.sai2b_get_body_contact_state(self.h, None, c))
        return c[3]

    # -- inverse kinematics (sai2b.h "inverse kinematics")
    def ik_config(self, **kwargs):
        """ik_config() of this module for this controller's model"""
        return ik_config(self.model, **kwargs)

    def set_ik(self, cfg=None, **kwargs):
        """the inverse kinematics of solve_ik(): an IkConfig (or the arguments of ik_config). Nothing else in the controller changes."""
        if cfg is None:
            cfg = self.ik_config(**kwargs)
        elif kwargs:
            raise ValueError("set_ik: an IkConfig or keyword arguments, not both")
        self._rc(self.lib.sai2b_set_ik(self.h, C.byref(cfg)))

    def clear_ik(self):
        self._rc(self.lib.sai2b_clear_ik(self.h))

    def get_ik(self):
        cfg = _abi.IkConfig()
        self._rc(self.lib.sai2b_get_ik(self.h, C.byref(cfg)))
        return cfg

    def ik_input_rows(self):
        """-> (rows of goal_rows, rows of seed_rows) that solve_ik() reads under the configuration in force"""
        cfg = self.get_ik()
        g, s = C.c_int(), C.c_int()
        self._rc(self.lib.sai2b_ik_input_rows(C.byref(cfg), self.dof, C.byref(g), C.byref(s)))
        return g.value, s.value

    def solve_ik(self, goal_rows=None, seed_rows=None, mask=None, q_out=None, status=None, flags=None):
        """one launch -> (q_out [dof][B], status [5][B] float64, flags [B] uint8 with the _abi.IK_FLAGS bits). goal_rows [12 (+ dof)][B]:
        position 3, rotation 9 row-major, then the rest posture when rest_weight > 0 (without the pose rows when the goal is the
        task's); seed_rows [dof][B] (None when the seed is the state); mask [B] bool / uint8, None: every robot. Everything numpy, or
        everything torch CUDA (then the three outputs are required, nothing leaves the device and nothing synchronises). Outputs not
        given are new numpy arrays of zeros; those given keep what the call does not write (unselected and non-finite robots)."""
        g_rows, s_rows = self.ik_input_rows()
        dev = self._dev(goal_rows, seed_rows, mask, q_out, status, flags)
        if dev and (q_out is None or status is None or flags is None):
            raise ValueError("solve_ik: with device tensors pass q_out, status and flags as tensors too")
        if (goal_rows is None) != (g_rows == 0) or (seed_rows is None) != (s_rows == 0):
            raise ValueError(f"solve_ik: the configuration reads {g_rows} goal rows and {s_rows} seed rows")
        pg, _kg = self._in(goal_rows, g_rows)
        ps, _ks = self._in(seed_rows, s_rows)
        pm, _km = self._mask(mask) if mask is not None else (None, None)
        if q_out is None:
            q_out = np.zeros((self.dof, self.B))
        if status is None:
            status = np.zeros((_abi.IK_STATUS_ROWS, self.B))
        if flags is None:
            flags = np.zeros(self.B, dtype=np.uint8)
        if dev:
            if str(flags.dtype) != "torch.uint8":
                raise ValueError("flags must be a uint8 tensor (it receives the flag bits)")
            pq, _ = self._in(q_out, self.dof)
            pst, _ = self._in(status, _abi.IK_STATUS_ROWS)
            pf, _ = self._mask(flags)
        else:
            for a, shape, dt, name in ((q_out, (self.dof, self.B), np.float64, "q_out"), (status, (_abi.IK_STATUS_ROWS, self.B), np.float64, "status"),
                                       (flags, (self.B,), np.uint8, "flags")):
                if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.shape == shape):
                    raise ValueError(f"{name} must be a C-contiguous {np.dtype(dt).name} array of shape {shape}")
            pq, pst, pf = (C.c_void_p(a.ctypes.data) for a in (q_out, status, flags))
        self._rc(self.lib.sai2b_solve_ik(self.h, pg, ps, pm, pq, pst, pf, dev))
        return q_out, status, flags

    def get_ik_counts(self):
        """of the last solve_ik(): dict 'selected', 'converged', 'exhausted', 'nonfinite' -> robots"""
        c = (C.c_int * 4)()
        self._rc(self.lib.sai2b_get_ik_counts(self.h, c))
        return dict(zip(_abi.IK_COUNTS, list(c)))

    # -- observations and episode-end flags (sai2b.h "observations and episode-end flags")
    @staticmethod
    def _flags(names, table, what):
        """iterable of names (or an int of flags) -> the or of the flags"""
        if isinstance(names, (int, np.integer)):
            return int(names)
        try:
            return sum({table[n] for n in names})
        except KeyError as e:
            raise ValueError(f"unknown {what} {e.args[0]!r}: one of {sorted(table)}") from None

    @staticmethod
    def _task_bits(tasks):
        if isinstance(tasks, (int, np.integer)) and not isinstance(tasks, bool):
            tasks = (tasks,)
        bits = 0
        for t in tasks:
            if not 0 <= int(t) < 31:
                raise ValueError(f"task index {t} out of range")
            bits |= 1 << int(t)
        return bits

    def observation_config(self, blocks=(), tasks=(), task_blocks=(), success_tasks=None, pos_tolerance=0.0, ori_tolerance=0.0,
                           joint_limit_margin=None, max_joint_speed=None, nonfinite=False, force_tasks=None, max_sensed_force=0.0,
                           max_episode_steps=None):
        """-> ObservationConfig. blocks: names of _abi.OBS_BLOCKS ('q', 'dq', 'tau', 'limit_margin', 'episode_step', 'contact');
        tasks: indices of the observed MotionForceTasks; task_blocks: names of _abi.OBS_TASK_BLOCKS ('pose', 'twist', 'error',
        'sensed'). A criterion is enabled by giving its argument: success_tasks (with pos_tolerance / ori_tolerance),
        joint_limit_margin, max_joint_speed (scalar or [dof]), nonfinite=True, force_tasks (with max_sensed_force),
        max_episode_steps."""
        cfg = _abi.ObservationConfig()
        rc = self.lib.sai2b_default_observation(C.byref(cfg))
        if rc:
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        cfg.blocks = self._flags(blocks, _abi.OBS_BLOCKS, "block")
        cfg.task_mask = self._task_bits(tasks)
        cfg.task_blocks = self._flags(task_blocks, _abi.OBS_TASK_BLOCKS, "task block")
        crit = 0
        if success_tasks is not None:
            crit |= _abi.DONE_SUCCESS
            cfg.success_task_mask = self._task_bits(success_tasks)
        cfg.pos_tolerance, cfg.ori_tolerance = float(pos_tolerance), float(ori_tolerance)
        if joint_limit_margin is not None:
            crit |= _abi.DONE_JOINT_LIMIT
            cfg.joint_limit_margin = float(joint_limit_margin)
        if max_joint_speed is not None:
            crit |= _abi.DONE_SPEED
            v = np.broadcast_to(np.asarray(max_joint_speed, dtype=np.float64), (self.dof,))
            for i in range(self.dof):
                cfg.max_joint_speed[i] = float(v[i])
        if nonfinite:
            crit |= _abi.DONE_NONFINITE
        if force_tasks is not None:
            crit |= _abi.DONE_FORCE
            cfg.force_task_mask = self._task_bits(force_tasks)
        cfg.max_sensed_force = float(max_sensed_force)
        if max_episode_steps is not None:
            crit |= _abi.DONE_TIMEOUT
            cfg.max_episode_steps = int(max_episode_steps)
        cfg.criteria = crit
        return cfg

    def set_observation(self, cfg=None, **kwargs):
        """configure what observe() stores and which criteria end an episode (an ObservationConfig, or the arguments of
        observation_config); every robot's episode counter restarts at zero"""
        if cfg is None:
            cfg = self.observation_config(**kwargs)
        elif kwargs:
            raise ValueError("set_observation: an ObservationConfig or keyword arguments, not both")
        self._rc(self.lib.sai2b_set_observation(self.h, C.byref(cfg)))

    def clear_observation(self):
        self._rc(self.lib.sai2b_clear_observation(self.h))

    def observation_rows(self):
        """rows of the configured observation; -1 without one"""
        return self.lib.sai2b_observation_rows(self.h)

    def observation_layout(self):
        """dict name -> slice of rows of observe()'s output: the global blocks by their names, the per-task blocks as
        'pose0', 'twist0', ... with the task index; only what the configuration stores"""
        first, n = C.c_int(), C.c_int()
        out = {}
        for name, flag in _abi.OBS_BLOCKS.items():
            self._rc(self.lib.sai2b_observation_layout(self.h, flag, -1, C.byref(first), C.byref(n)))
            if n.value:
                out[name] = slice(first.value, first.value + n.value)
        for t in range(len(self.tasks)):
            for name, flag in _abi.OBS_TASK_BLOCKS.items():
                self._rc(self.lib.sai2b_observation_layout(self.h, flag, t, C.byref(first), C.byref(n)))
                if n.value:
                    out[f"{name}{t}"] = slice(first.value, first.value + n.value)
        return out

    def observe(self, out=None, done=None):
        """one launch -> (rows [observation_rows()][B] float64, done [B] uint8 with the _abi.DONE_* bits). out / done: numpy
        arrays or torch CUDA tensors to fill (both of one kind; a torch pair never leaves the device and nothing synchronises),
        None: a new numpy array, False: not wanted (None is returned in its place)"""
        rows = self.observation_rows()
        if rows < 0:
            raise ValueError("sai2b_observe: no observation is configured (sai2b_set_observation)")
        given = [o for o in (out, done) if o is not None and o is not False]
        dev = self._dev(*given)
        if dev and (out is None or done is None):
            raise ValueError("observe: with a device tensor pass the other argument as a tensor too, or False")
        if out is None:
            out = np.empty((rows, self.B))
        if done is None:
            done = np.zeros(self.B, dtype=np.uint8)
        po = pd = None
        if out is not False:
            if hasattr(out, "data_ptr"):
                po, _ = self._in(out, rows)
            else:
                if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (rows, self.B)):
                    raise ValueError(f"out must be a C-contiguous float64 array of shape ({rows}, {self.B})")
                po = C.c_void_p(out.ctypes.data)
        if done is not False:
            if hasattr(done, "data_ptr"):
                if str(done.dtype) != "torch.uint8":
                    raise ValueError("done must be a uint8 tensor (it receives the reason bits)")
                pd, _ = self._mask(done)
            else:
                if not (isinstance(done, np.ndarray) and done.dtype == np.uint8 and done.flags.c_contiguous and done.shape == (self.B,)):
                    raise ValueError(f"done must be a C-contiguous uint8 array of shape ({self.B},)")
                pd = C.c_void_p(done.ctypes.data)
        self._rc(self.lib.sai2b_observe(self.h, po, pd, dev))
        return (None if out is False else out), (None if done is False else done)

    def done_counts(self):
        """of the last observe(): dict reason name -> robots with that bit, and 'any' -> robots with a non-zero byte"""
        c = (C.c_int * 7)()
        self._rc(self.lib.sai2b_get_done_counts(self.h, c))
        return dict(zip(list(_abi.DONE_BITS) + ["any"], list(c)))

    # -- rewards and episode returns (sai2b.h "rewards and episode returns")
    def reward_config(self, terms=None, tasks=None, done_value=None, limit_soft_margin=0.0, gamma=1.0, nonfinite_reward=0.0):
        """-> RewardConfig. terms: dict name of _abi.REW_TERMS ('alive', 'joint_speed', 'torque', 'torque_rate', 'limit', 'done')
        -> weight. tasks: dict MotionForceTask index -> dict of that task's settings: 'terms': dict name of _abi.REW_TASK_TERMS
        ('pos', 'pos_sq', 'pos_tanh', 'ori', 'ori_sq', 'ori_tanh', 'lin_vel_sq', 'ang_vel_sq', 'force_err_sq', 'force_excess') ->
        weight, and pos_scale, ori_scale, force_soft_limit. The configuration is batch-uniform and every task evaluates the same
        set of terms: the union over the tasks, with weight 0 where a task does not name one. done_value: dict reason name of
        _abi.DONE_BITS -> value of the 'done' term."""
        cfg = _abi.RewardConfig()
        rc = self.lib.sai2b_default_reward(C.byref(cfg))
        if rc:
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        names = list(_abi.REW_TERMS)
        for name, w in (terms or {}).items():
            cfg.terms |= self._flags((name,), _abi.REW_TERMS, "reward term")
            cfg.weight[names.index(name)] = float(w)
        tnames = list(_abi.REW_TASK_TERMS)
        for t, spec in (tasks or {}).items():
            t = int(t)
            if not 0 <= t < _abi.MAX_TASKS:
                raise ValueError(f"task index {t} out of range")
            spec = dict(spec)
            cfg.task_mask |= 1 << t
            for name, w in spec.pop("terms", {}).items():
                cfg.task_terms |= self._flags((name,), _abi.REW_TASK_TERMS, "reward task term")
                cfg.task_weight[t][tnames.index(name)] = float(w)
            for key in ("pos_scale", "ori_scale", "force_soft_limit"):
                if key in spec:
                    getattr(cfg, key)[t] = float(spec.pop(key))
            if spec:
                raise ValueError(f"reward_config: unknown task setting(s) {sorted(spec)}")
        reasons = list(_abi.DONE_BITS)
        for name, v in (done_value or {}).items():
            if name not in _abi.DONE_BITS:
                raise ValueError(f"unknown done reason {name!r}: one of {reasons}")
            cfg.done_value[reasons.index(name)] = float(v)
        cfg.limit_soft_margin, cfg.gamma, cfg.nonfinite_reward = float(limit_soft_margin), float(gamma), float(nonfinite_reward)
        return cfg

    def set_reward(self, cfg=None, **kwargs):
        """configure what observe_reward() evaluates (a RewardConfig, or the arguments of reward_config); needs a configured
        observation; every robot's accumulators restart (return 0, discount 1, no last episode, no tau_prev)"""
        if cfg is None:
            cfg = self.reward_config(**kwargs)
        elif kwargs:
            raise ValueError("set_reward: a RewardConfig or keyword arguments, not both")
        self._rc(self.lib.sai2b_set_reward(self.h, C.byref(cfg)))

    def clear_reward(self):
        self._rc(self.lib.sai2b_clear_reward(self.h))

    def reward_rows(self):
        """rows of the configured reward's terms; -1 without one"""
        return self.lib.sai2b_reward_rows(self.h)

    def reward_layout(self):
        """dict name -> row of observe_reward()'s terms: the global terms by their names, the task terms as 'pos0',
        'force_err_sq1', ... with the task index; only what the configuration selects"""
        first, n = C.c_int(), C.c_int()
        out = {}
        for name, flag in _abi.REW_TERMS.items():
            self._rc(self.lib.sai2b_reward_layout(self.h, flag, -1, C.byref(first), C.byref(n)))
            if n.value:
                out[name] = first.value
        for t in range(len(self.tasks)):
            for name, flag in _abi.REW_TASK_TERMS.items():
                self._rc(self.lib.sai2b_reward_layout(self.h, flag, t, C.byref(first), C.byref(n)))
                if n.value:
                    out[f"{name}{t}"] = first.value
        return out

    def observe_reward(self, out=None, done=None, reward=None, terms=False):
        """observe() and the reward in one launch -> (rows, done, reward [B] float64, terms [reward_rows()][B] float64). Every
        argument: a numpy array or a torch CUDA tensor to fill (all of one kind; torch arguments never leave the device and
        nothing synchronises), None: a new numpy array, False: not wanted (None is returned in its place). The accumulators
        advance whatever is wanted."""
        rows, rrows = self.observation_rows(), self.reward_rows()
        if rows < 0:
            raise ValueError("sai2b_observe_reward: no observation is configured (sai2b_set_observation)")
        if rrows < 0:
            raise ValueError("sai2b_observe_reward: no reward is configured (sai2b_set_reward)")
        args = (out, done, reward, terms)
        dev = self._dev(*[o for o in args if o is not None and o is not False])
        if dev and any(o is None for o in args):
            raise ValueError("observe_reward: with a device tensor pass every other argument as a tensor too, or False")
        if out is None:
            out = np.empty((rows, self.B))
        if done is None:
            done = np.zeros(self.B, dtype=np.uint8)
        if reward is None:
            reward = np.empty(self.B)
        if terms is None:
            terms = np.empty((rrows, self.B))

        def rows_ptr(a, n, name, flat=False):
            if a is False:
                return None
            shape = (self.B,) if flat else (n, self.B)
            if hasattr(a, "data_ptr"):
                if tuple(a.shape) != shape:
                    raise ValueError(f"{name} must be a tensor of shape {shape}")
                return self._in(a.view(n, self.B), n)[0]
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == shape):
                raise ValueError(f"{name} must be a C-contiguous float64 array of shape {shape}")
            return C.c_void_p(a.ctypes.data)

        po = rows_ptr(out, rows, "out")
        pr = rows_ptr(reward, 1, "reward", flat=True)
        pt = rows_ptr(terms, rrows, "terms")
        pd = None
        if done is not False:
            if hasattr(done, "data_ptr"):
                if str(done.dtype) != "torch.uint8":
                    raise ValueError("done must be a uint8 tensor (it receives the reason bits)")
                pd, _ = self._mask(done)
            else:
                if not (isinstance(done, np.ndarray) and done.dtype == np.uint8 and done.flags.c_contiguous and done.shape == (self.B,)):
                    raise ValueError(f"done must be a C-contiguous uint8 array of shape ({self.B},)")
                pd = C.c_void_p(done.ctypes.data)
        self._rc(self.lib.sai2b_observe_reward(self.h, po, pd, pr, pt, dev))
        return tuple(None if o is False else o for o in (out, done, reward, terms))

    def reward_counts(self):
        """of the last observe_reward(): dict 'closed' -> robots whose episode was closed, 'replaced' -> robots whose reward was
        not finite and became nonfinite_reward"""
        c = (C.c_int * 2)()
        self._rc(self.lib.sai2b_get_reward_counts(self.h, c))
        return dict(zip(_abi.REW_COUNTS, list(c)))

    def episode_stats(self):
        """the accumulators as they are now: dict of [B] arrays ret, discount, last_return (float64) and last_length (int32)"""
        r, d, l = np.empty(self.B), np.empty(self.B), np.empty(self.B)
        n = np.empty(self.B, dtype=np.int32)
        self._rc(self.lib.sai2b_get_episode_stats(self.h, *[C.c_void_p(a.ctypes.data) for a in (r, d, l, n)]))
        return dict(ret=r, discount=d, last_return=l, last_length=n)

    def reward_state(self):
        """the two device buffers as torch views (no copy): state [3 + dof][B] float64 = ret, disc, last_return, tau_prev and
        episode [2][B] int32 = last_length, tau_prev_valid. Order reads and writes with stream()."""
        import torch

        ps, pe = self.device_buffer(_abi.BUF_REWARD_STATE), self.device_buffer(_abi.BUF_REWARD_EPISODE)
        if not ps or not pe:
            raise ValueError("reward_state: no reward is configured (sai2b_set_reward)")

        def view(ptr, rows, typestr, dtype):
            class _Buf:
                __cuda_array_interface__ = dict(shape=(rows, self.B), typestr=typestr, data=(int(ptr), False), version=2)

            return torch.as_tensor(_Buf(), device=f"cuda:{self._device}").view(dtype)

        return view(ps, 3 + self.dof, "<f8", torch.float64), view(pe, 2, "<i4", torch.int32)

    # -- actions (sai2b.h "actions")
    def action_config(self, tasks=None, clip_actions=False):
        """-> ActionConfig. tasks: dict task index -> dict of that task's settings, every other task takes no rows:
        mode ('delta_goal', 'delta_current', 'absolute'), for a MotionForceTask blocks (names of _abi.ACT_BLOCKS: 'position',
        'orientation', 'force', 'moment'), pos_scale / pos_lower / pos_upper (scalar or [3]), ori_scale, force_scale,
        moment_scale, max_pos_lead; for a JointTask jt_scale / jt_lower / jt_upper (scalar or [task_dof]) or
        jt_limits='model': the model's joint limits (a full joint task only)."""
        cfg = _abi.ActionConfig()
        if self.lib.sai2b_default_action(C.byref(cfg)):
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        cfg.clip_actions = int(bool(clip_actions))
        for t, settings in dict(tasks or {}).items():
            if not 0 <= int(t) < _abi.MAX_TASKS:
                raise ValueError(f"task index {t} out of range")
            a, s = cfg.task[int(t)], dict(settings)
            mode = s.pop("mode", "none")
            if isinstance(mode, str) and mode not in _abi.ACT_MODES:
                raise ValueError(f"unknown mode {mode!r}: one of {sorted(_abi.ACT_MODES)}")
            a.mode = _abi.ACT_MODES[mode] if isinstance(mode, str) else int(mode)
            a.blocks = self._flags(s.pop("blocks", ()), _abi.ACT_BLOCKS, "block")
            k0 = self.tasks[int(t)].task_dof if int(t) < len(self.tasks) and self.tasks[int(t)].type == _abi.JOINT_TASK else 0
            if "jt_limits" in s:
                if s.pop("jt_limits") != "model" or "jt_lower" in s or "jt_upper" in s:
                    raise ValueError("jt_limits must be 'model', without jt_lower / jt_upper")
                if k0 != self.dof:
                    raise ValueError("jt_limits='model' is for a full joint task")
                s["jt_lower"], s["jt_upper"] = list(self.model.q_lower)[:k0], list(self.model.q_upper)[:k0]
            for name in ("pos_scale", "pos_lower", "pos_upper", "jt_scale", "jt_lower", "jt_upper"):
                if name in s:
                    n = 3 if name.startswith("pos") else k0
                    v = np.broadcast_to(np.asarray(s.pop(name), dtype=np.float64), (n,))
                    for i in range(n):
                        getattr(a, name)[i] = float(v[i])
            for name in ("ori_scale", "force_scale", "moment_scale", "max_pos_lead"):
                if name in s:
                    setattr(a, name, float(s.pop(name)))
            if s:
                raise ValueError(f"unknown action setting {sorted(s)[0]!r} of task {t}")
        return cfg

    def set_action(self, cfg=None, **kwargs):
        """configure what apply_action() maps (an ActionConfig, or the arguments of action_config)"""
        if cfg is None:
            cfg = self.action_config(**kwargs)
        elif kwargs:
            raise ValueError("set_action: an ActionConfig or keyword arguments, not both")
        self._rc(self.lib.sai2b_set_action(self.h, C.byref(cfg)))

    def clear_action(self):
        self._rc(self.lib.sai2b_clear_action(self.h))

    def action_rows(self):
        """rows of the configured action; -1 without one"""
        return self.lib.sai2b_action_rows(self.h)

    def action_layout(self):
        """dict name -> slice of rows of the action: 'position0', 'orientation0', 'force0', 'moment0' with the index of the
        MotionForceTask, 'joints1' with that of the JointTask; only what the configuration reads"""
        first, n = C.c_int(), C.c_int()
        out = {}
        for t, task in enumerate(self.tasks):
            blocks = {"joints": _abi.ACT_POSITION} if task.type == _abi.JOINT_TASK else _abi.ACT_BLOCKS
            for name, flag in blocks.items():
                self._rc(self.lib.sai2b_action_layout(self.h, flag, t, C.byref(first), C.byref(n)))
                if n.value:
                    out[f"{name}{t}"] = slice(first.value, first.value + n.value)
        return out

    def apply_action(self, action, mask=None):
        """one launch: action [action_rows()][B] to the goal rows of the configured tasks, for the robots mask selects ([B]
        bool / uint8, None: every robot). numpy arrays, or torch CUDA tensors (then nothing leaves the device and nothing
        synchronises)"""
        rows = self.action_rows()
        if rows < 0:
            raise ValueError("sai2b_apply_action: no action is configured (sai2b_set_action)")
        dev = self._dev(action, mask)
        pa, ka = self._in(action, rows)
        if pa is None:
            raise ValueError(f"an action of shape ({rows}, {self.B}) is required")
        pm, km = self._mask(mask) if mask is not None else (None, None)
        self._rc(self.lib.sai2b_apply_action(self.h, pa, pm, dev))

    def action_counts(self):
        """of the last apply_action(): dict 'rejected', 'clipped', 'limited' -> robots"""
        c = (C.c_int * 3)()
        self._rc(self.lib.sai2b_get_action_counts(self.h, c))
        return dict(zip(_abi.ACT_COUNTS, list(c)))

    # -- the path
    def reinitialize(self):
        self._rc(self.lib.sai2b_reinitialize(self.h))

    def _mask(self, mask):
        """-> (pointer, keepalive) for a [B] mask: numpy bool / uint8 array or contiguous torch CUDA bool / uint8 tensor"""
        if mask is None:
            raise ValueError("a mask of one entry per robot is required")
        if hasattr(mask, "data_ptr"):  # torch tensor
            if not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != (self.B,) or str(mask.dtype) not in ("torch.bool", "torch.uint8"):
                raise ValueError(f"expected a contiguous bool or uint8 CUDA tensor of shape ({self.B},)")
            import torch

            s = torch.cuda.current_stream(mask.device).cuda_stream
            if s != self._caller_stream:
                self._rc(self.lib.sai2b_set_caller_stream(self.h, C.c_void_p(s)))
                self._caller_stream = s
            return C.c_void_p(mask.data_ptr()), mask
        arr = np.asarray(mask)
        if arr.dtype not in (np.bool_, np.uint8):
            raise ValueError(f"expected a bool or uint8 mask, got dtype {arr.dtype}")
        if arr.shape != (self.B,):
            raise ValueError(f"expected a mask of shape ({self.B},), got {arr.shape}")
        arr = np.ascontiguousarray(arr).view(np.uint8)
        return C.c_void_p(arr.ctypes.data), arr

    def reinitialize_robots(self, mask, task=-1):
        """reinitialize() (task = -1) or task_reinitialize(task) for the robots the mask selects; the others are not touched"""
        task = int(task)
        if not (-1 <= task < len(self.tasks)):
            raise ValueError(f"task must be -1 (every task) or a task index below {len(self.tasks)}")
        pm, km = self._mask(mask)
        self._rc(self.lib.sai2b_reinitialize_robots(self.h, task, pm, self._dev(mask)))

    def reset_robots(self, mask, q=None, dq=None):
        """Episode reset of the robots the mask selects: the selected columns of q, dq ([dof][B], None = keep) become their
        state, their tasks and passivity observers are re-initialised and their stored torques zeroed; the others are not
        touched. Mask and rows all numpy or all torch CUDA (then nothing synchronises)."""
        pm, km = self._mask(mask)
        pq, kq = self._in(q, self.dof)
        pd, kd = self._in(dq, self.dof)
        self._rc(self.lib.sai2b_reset_robots(self.h, pm, pq, pd, self._dev(mask, q, dq)))

    # -- episode starts (sai2b.h "episode starts")
    def reset_sampler_config(self, seed=0, first_robot=0, max_tries=8, goal_tasks=(), absolute_position=(), ratio_task=-1, min_ratio=0.0,
                             box_task=-1, box_lower=(0.0, 0.0, 0.0), box_upper=(0.0, 0.0, 0.0), clearance=None):
        """-> ResetSamplerConfig, validated against this controller's tasks. goal_tasks / absolute_position: task indices (or an
        int of bits); ratio_task, min_ratio: the singularity criterion; box_task, box_lower, box_upper: the workspace box;
        clearance: metres over the contact plane (None: no clearance criterion)"""
        cfg = _abi.ResetSamplerConfig()
        if self.lib.sai2b_default_reset_sampler(C.byref(cfg)):
            raise ValueError(self.lib.sai2b_last_error(None).decode())

        def bits(v):
            if isinstance(v, (int, np.integer)):
                return int(v) & 0xFFFFFFFF
            out = 0
            for t in v:
                if not 0 <= int(t) < 32:
                    raise ValueError(f"reset sampler: task index {t} out of range")
                out |= 1 << int(t)
            return out

        cfg.seed, cfg.first_robot, cfg.max_tries = int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_robot) & 0xFFFFFFFF, int(max_tries)
        cfg.goal_tasks, cfg.absolute_position = bits(goal_tasks), bits(absolute_position)
        cfg.ratio_task, cfg.min_ratio, cfg.box_task = int(ratio_task), float(min_ratio), int(box_task)
        lo, hi = np.asarray(box_lower, dtype=np.float64), np.asarray(box_upper, dtype=np.float64)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("box_lower, box_upper: expected 3 values each")
        cfg.box_lower[:], cfg.box_upper[:] = [float(x) for x in lo], [float(x) for x in hi]
        cfg.use_clearance, cfg.clearance = (0, 0.0) if clearance is None else (1, float(clearance))
        msg = C.create_string_buffer(256)
        tasks = (_abi.TaskConfig * len(self.tasks))(*self.tasks)
        if self.lib.sai2b_validate_reset_sampler(C.byref(cfg), tasks, len(self.tasks), self.dof, msg, 256):
            # (for a robot size without a build the dispatcher answers and leaves msg empty: its text is the shared error's)
            raise ValueError(msg.value.decode() or self.lib.sai2b_last_error(None).decode())
        return cfg

    def reset_sampler_layout(self, cfg):
        """dict name -> (first_row, n_rows) of the per-robot rows of `cfg`: 'q_lower', 'q_upper', 'dq_sigma', 'q_nominal' and
        'goal<t>' for every task of goal_tasks; 'total' -> rows of the whole buffer"""
        tasks = (_abi.TaskConfig * len(self.tasks))(*self.tasks)
        first, n, total = C.c_int(), C.c_int(), C.c_int()
        out = {}
        for name, block in _abi.RESET_SAMPLER_BLOCKS.items():
            for t in range(len(self.tasks)) if name == "goal" else (0,):
                rc = self.lib.sai2b_reset_sampler_config_layout(C.byref(cfg), tasks, len(self.tasks), self.dof, block, t, C.byref(first),
                                                                C.byref(n), C.byref(total))
                if rc:
                    raise ValueError(self.lib.sai2b_last_error(None).decode())
                if n.value:
                    out[f"goal{t}" if name == "goal" else name] = (first.value, n.value)
        out["total"] = total.value
        return out

    def reset_sampler_rows(self, cfg, q_lower=None, q_upper=None, dq_sigma=0.0, q_nominal=None, goals=None):
        """-> rows [total][B] (numpy) for `cfg`. q_lower, q_upper, q_nominal (None: the defaults: the middle 80 % of the joint range
        and its middle), dq_sigma: a scalar, [dof] values or [dof][B]. goals: dict task -> dict(pos_lower=, pos_upper=, theta_max=)
        for a MotionForceTask ([3] / scalar or [..][B]) or dict(half_width=) for a JointTask; what is left out is 0"""
        n, B = self.dof, self.B
        lay = self.reset_sampler_layout(cfg)
        lo_m = np.array([self.model.q_lower[i] for i in range(n)])
        hi_m = np.array([self.model.q_upper[i] for i in range(n)])
        mid, half = 0.5 * (lo_m + hi_m), 0.5 * (hi_m - lo_m)

        def block(a, rows, name):
            a = np.asarray(a, dtype=np.float64)
            if a.ndim == 1 and a.shape[0] == rows and rows != B:
                a = a[:, None]
            try:
                return np.broadcast_to(a, (rows, B))
            except ValueError:
                raise ValueError(f"{name}: expected a scalar, {rows} values or an array of shape ({rows}, {B})") from None

        rows = np.zeros((lay["total"], B))
        rows[0:n] = block(mid - 0.8 * half if q_lower is None else q_lower, n, "q_lower")
        rows[n : 2 * n] = block(mid + 0.8 * half if q_upper is None else q_upper, n, "q_upper")
        rows[2 * n : 3 * n] = block(dq_sigma, n, "dq_sigma")
        rows[3 * n : 4 * n] = block(mid if q_nominal is None else q_nominal, n, "q_nominal")
        for t, spec in (goals or {}).items():
            key = f"goal{int(t)}"
            if key not in lay:
                raise ValueError(f"reset_sampler_rows: task {t} is not in goal_tasks")
            first, cnt = lay[key]
            spec = dict(spec)
            if self.tasks[int(t)].type == _abi.MOTION_FORCE_TASK:
                rows[first : first + 3] = block(spec.pop("pos_lower", 0.0), 3, "pos_lower")
                rows[first + 3 : first + 6] = block(spec.pop("pos_upper", 0.0), 3, "pos_upper")
                rows[first + 6] = np.broadcast_to(np.asarray(spec.pop("theta_max", 0.0), dtype=np.float64), (B,))
            else:
                rows[first : first + cnt] = block(spec.pop("half_width", 0.0), cnt, "half_width")
            if spec:
                raise ValueError(f"reset_sampler_rows: unknown setting(s) {sorted(spec)} for task {t}")
        return rows

    def set_reset_sampler(self, cfg=None, rows=None, **kwargs):
        """configure what reset_robots_sampled() draws: a ResetSamplerConfig (or the arguments of reset_sampler_config) and the
        per-robot rows [total][B], numpy (validated) or torch CUDA (not inspected), None = the defaults. Zeroes the episode
        counters."""
        if cfg is None:
            cfg = self.reset_sampler_config(**kwargs)
        elif kwargs:
            raise ValueError("set_reset_sampler: a ResetSamplerConfig or keyword arguments, not both")
        total = self.reset_sampler_layout(cfg)["total"]
        if rows is not None and not hasattr(rows, "data_ptr"):
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            if rows.shape != (total, self.B):
                raise ValueError(f"rows: expected an array of shape ({total}, {self.B})")
        pr, keep = self._in(rows, total)
        self._rc(self.lib.sai2b_set_reset_sampler(self.h, C.byref(cfg), pr, self._dev(rows)))

    def clear_reset_sampler(self):
        self._rc(self.lib.sai2b_clear_reset_sampler(self.h))

    def get_reset_sampler(self):
        """-> (ResetSamplerConfig, rows [total][B])"""
        cfg = _abi.ResetSamplerConfig()
        self._rc(self.lib.sai2b_get_reset_sampler(self.h, C.byref(cfg), None))
        rows = np.empty((self.reset_sampler_layout(cfg)["total"], self.B))
        self._rc(self.lib.sai2b_get_reset_sampler(self.h, None, C.c_void_p(rows.ctypes.data)))
        return cfg, rows

    def reset_robots_sampled(self, mask):
        """reset_robots() for the robots the mask selects with their start state and goals drawn on the device (sai2b.h "episode
        starts"); mask numpy or torch CUDA (then nothing synchronises)"""
        pm, km = self._mask(mask)  # (None: ValueError)
        self._rc(self.lib.sai2b_reset_robots_sampled(self.h, pm, self._dev(mask)))

    def reset_sampler_counts(self):
        """of the last reset_robots_sampled(): dict 'reset' -> robots reset, 'rejected' -> candidates rejected, 'exhausted' ->
        robots that got q_nominal"""
        c = (C.c_int * 3)()
        self._rc(self.lib.sai2b_get_reset_sampler_counts(self.h, c))
        return dict(zip(_abi.RESET_SAMPLER_COUNTS, (int(x) for x in c)))

    def reset_sampler_state(self):
        """-> dict episode [B], tries [B] (int32): the episode counter, the candidates used by the call that reset the robot last"""
        e, t = np.empty(self.B, dtype=np.int32), np.empty(self.B, dtype=np.int32)
        self._rc(self.lib.sai2b_get_reset_sampler_state(self.h, C.c_void_p(e.ctypes.data), C.c_void_p(t.ctypes.data)))
        return dict(episode=e, tries=t)

    # -- environment sampler (sai2b.h "environment sampler")
    def env_sampler_config(self, seed=0, first_robot=0, groups=(), payload_target="plant", **kw):
        """-> EnvSamplerConfig, validated. groups: names of _abi.ENV_GROUPS (or an int of bits). Every other field of
        sai2b_env_sampler_config by its name: a range as (lower, upper), (lower, upper, log_uniform) or one number for both
        bounds; payload_com_half [3], sensor_bias_half [6] as sequences or one number; the rest as numbers"""
        cfg = _abi.EnvSamplerConfig()
        if self.lib.sai2b_default_env_sampler(C.byref(cfg)):
            raise ValueError(self.lib.sai2b_last_error(None).decode())
        cfg.seed, cfg.first_robot = int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_robot) & 0xFFFFFFFF
        if isinstance(groups, (int, np.integer)):
            cfg.groups = int(groups) & 0xFFFFFFFF
        else:
            for g in [groups] if isinstance(groups, str) else groups:
                if g not in _abi.ENV_GROUPS:
                    raise ValueError(f"env sampler: unknown group {g!r} (one of {sorted(_abi.ENV_GROUPS)})")
                cfg.groups |= _abi.ENV_GROUPS[g]
        cfg.payload_target = _abi.PAYLOAD_TARGETS[payload_target] if isinstance(payload_target, str) else int(payload_target)
        for name, v in kw.items():
            if name in _abi.ENV_RANGE_FIELDS:
                v = (v, v) if np.isscalar(v) else tuple(v)
                if len(v) not in (2, 3):
                    raise ValueError(f"{name}: expected (lower, upper) or (lower, upper, log_uniform)")
                r = getattr(cfg, name)
                r.lower, r.upper, r.log_uniform = float(v[0]), float(v[1]), int(bool(v[2])) if len(v) == 3 else 0
            elif name in ("payload_com_half", "sensor_bias_half"):
                n = 3 if name == "payload_com_half" else 6
                a = np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))
                getattr(cfg, name)[:] = [float(x) for x in a]
            elif name == "contact_tilt_max":
                cfg.contact_tilt_max = float(v)
            elif name in ("delay_lower", "delay_upper", "push_steps_lower", "push_steps_upper"):
                setattr(cfg, name, int(v))
            else:
                raise ValueError(f"env sampler: unknown setting {name!r}")
        msg = C.create_string_buffer(256)
        if self.lib.sai2b_validate_env_sampler(C.byref(cfg), self.dof, msg, 256):
            raise ValueError(msg.value.decode() or self.lib.sai2b_last_error(None).decode())
        return cfg

    def env_sampler_layout(self, cfg):
        """dict group name -> (first_row, n_rows) of the sample rows of `cfg` (its configured groups); 'total' -> rows of the buffer"""
        first, n, total = C.c_int(), C.c_int(), C.c_int()
        out = {}
        for name, bit in _abi.ENV_GROUPS.items():
            if self.lib.sai2b_env_sampler_config_layout(C.byref(cfg), self.dof, bit, C.byref(first), C.byref(n), C.byref(total)):
                raise ValueError(self.lib.sai2b_last_error(None).decode())
            if n.value:
                out[name] = (first.value, n.value)
        out["total"] = total.value
        return out

    def set_env_sampler(self, cfg=None, **kwargs):
        """configure what randomize_robots() draws: an EnvSamplerConfig (or the arguments of env_sampler_config). The rows of
        the features of its groups as they are now become the nominal every draw starts from; zeroes the draw counters"""
        if cfg is None:
            cfg = self.env_sampler_config(**kwargs)
        elif kwargs:
            raise ValueError("set_env_sampler: an EnvSamplerConfig or keyword arguments, not both")
        self._rc(self.lib.sai2b_set_env_sampler(self.h, C.byref(cfg)))

    def clear_env_sampler(self):
        self._rc(self.lib.sai2b_clear_env_sampler(self.h))

    def get_env_sampler(self):
        """-> the EnvSamplerConfig in force"""
        cfg = _abi.EnvSamplerConfig()
        self._rc(self.lib.sai2b_get_env_sampler(self.h, C.byref(cfg)))
        return cfg

    def randomize_robots(self, mask, groups=0):
        """redraw the plant of the robots the mask selects (sai2b.h "environment sampler"); groups: names of _abi.ENV_GROUPS or
        an int of bits, 0 = every configured group; mask numpy or torch CUDA (then nothing synchronises)"""
        if not isinstance(groups, (int, np.integer)):
            groups = sum({_abi.ENV_GROUPS[g] for g in ([groups] if isinstance(groups, str) else groups)})
        pm, km = self._mask(mask)  # (None: ValueError)
        self._rc(self.lib.sai2b_randomize_robots(self.h, pm, int(groups) & 0xFFFFFFFF, self._dev(mask)))

    def env_sampler_counts(self):
        """of the last randomize_robots(): dict 'drawn' -> robots drawn, 'lag_clipped' -> robots with a lag clipped at 1"""
        c = (C.c_int * 2)()
        self._rc(self.lib.sai2b_get_env_sampler_counts(self.h, c))
        return dict(zip(_abi.ENV_SAMPLER_COUNTS, (int(x) for x in c)))

    def env_sampler_state(self):
        """-> dict counter [B] (int32): the draw counter, sample [total][B]: what the last draws were"""
        total = self.env_sampler_layout(self.get_env_sampler())["total"]
        c, s = np.empty(self.B, dtype=np.int32), np.zeros((total, self.B))
        self._rc(self.lib.sai2b_get_env_sampler_state(self.h, C.c_void_p(c.ctypes.data), C.c_void_p(s.ctypes.data) if total else None))
        return dict(counter=c, sample=s)

    # -- snapshot banks (sai2b.h "snapshot banks")
    def snapshot_words(self, what=_abi.SNAP_EPISODE):
        """4-byte words of one robot's state for this controller as configured now"""
        n = self.lib.sai2b_snapshot_words(self.h, int(what))
        if n < 0:
            self._rc(_abi.INVALID_ARGUMENT)
        return n

    def snapshot_layout(self, what=_abi.SNAP_EPISODE):
        """the row table behind snapshot_words(): list of dicts block (name), task (-1: none), rows, elem_bytes, first_word"""
        tab = (C.c_int * (5 * 80))()
        n = self.lib.sai2b_snapshot_layout(self.h, int(what), tab, 80)
        if n < 0:
            self._rc(_abi.INVALID_ARGUMENT)
        return [dict(block=_abi.SNAP_BLOCK_NAMES_ALL[tab[5 * i]], task=tab[5 * i + 1], rows=tab[5 * i + 2], elem_bytes=tab[5 * i + 3],
                     first_word=tab[5 * i + 4]) for i in range(n)]

    def snapshot_bank(self, capacity, what=_abi.SNAP_EPISODE):
        """a SnapshotBank of `capacity` slots for the state groups `what` (SNAP_EPISODE | SNAP_ENVIRONMENT)"""
        return SnapshotBank(self, capacity, what)

    def _slots(self, slots):
        """-> (pointer, keepalive) for [B] slot indices: numpy integer array or contiguous torch CUDA int32 tensor"""
        if hasattr(slots, "data_ptr"):  # torch tensor
            if not slots.is_cuda or not slots.is_contiguous() or tuple(slots.shape) != (self.B,) or str(slots.dtype) != "torch.int32":
                raise ValueError(f"expected a contiguous int32 CUDA tensor of shape ({self.B},)")
            import torch

            s = torch.cuda.current_stream(slots.device).cuda_stream
            if s != self._caller_stream:
                self._rc(self.lib.sai2b_set_caller_stream(self.h, C.c_void_p(s)))
                self._caller_stream = s
            return C.c_void_p(slots.data_ptr()), slots
        arr = np.asarray(slots)
        if arr.dtype.kind not in "iu":
            raise ValueError(f"expected integer slots, got dtype {arr.dtype}")
        if arr.shape != (self.B,):
            raise ValueError(f"expected slots of shape ({self.B},), got {arr.shape}")
        arr = np.ascontiguousarray(np.clip(arr, -1, 2**31 - 1), dtype=np.int32)  # (anything out of range stays out of range)
        return C.c_void_p(arr.ctypes.data), arr

    def update_task_models(self):
        self._rc(self.lib.sai2b_update_task_models(self.h))

    def compute_control_torques(self, with_compensation=True, out=None):
        return self._torques(lambda p, dev: self.lib.sai2b_compute_control_torques_ex(self.h, p, dev, int(with_compensation)), out)

    def tick(self, out=None, want_output=True):
        """fused update_task_models + compute_control_torques; with want_output=False only enqueues"""
        if not want_output:
            self._rc(self.lib.sai2b_tick(self.h, None, 0))
            return None
        return self._torques(lambda p, dev: self.lib.sai2b_tick(self.h, p, dev), out)

    def _torques(self, call, out):
        if out is None:
            out = np.empty((self.dof, self.B))
        p, keep = self._in(out, self.dof)
        if not hasattr(out, "data_ptr") and keep is not out:
            raise ValueError("out must be a C-contiguous float64 array")
        self._rc(call(p, self._dev(out)))
        return out

    # -- task-level plugin interface (TemplateTask.h:42-88): one task driven on its own
    def task_update_model(self, task, N_prec=None):
        """TemplateTask::updateTaskModel(N_prec); N_prec [n*n][B] (numpy or torch CUDA), None = identity"""
        p, _ = self._in(N_prec, self.dof * self.dof)
        self._rc(self.lib.sai2b_task_update_model(self.h, task, p, self._dev(N_prec)))

    def task_update_model_behind(self, task, previous_task):
        """updateTaskModel(previous->getTaskAndPreviousNullspace()) without the host round trip of the [n*n][B] matrix:
        the previous task's N * N_prec is read where its own update left it on the device (same context, same stream)"""
        p = self.lib.sai2b_device_buffer(self.h, _abi.BUF_TASK_N_TOTAL, int(previous_task))
        if not p:
            raise ValueError("task_update_model_behind: the previous task has no task-level model yet")
        self._rc(self.lib.sai2b_task_update_model(self.h, task, C.c_void_p(p), 1))

    def task_compute_torques(self, task, tau_prec=None, out=None):
        """TemplateTask::computeTorques() / computeTorques(tau_prec): the task's own torques [n][B]"""
        p, _ = self._in(tau_prec, self.dof)
        if out is None:
            out = np.empty((self.dof, self.B))
        po, keep = self._in(out, self.dof)
        if tau_prec is not None and self._dev(tau_prec) != self._dev(out):
            raise ValueError("tau_prec and out must both be host arrays or both device tensors")
        self._rc(self.lib.sai2b_task_compute_torques(self.h, task, p, po, self._dev(out)))
        return out

    def task_reinitialize(self, task):
        self._rc(self.lib.sai2b_task_reinitialize(self.h, task))

    def task_nullspaces(self, task):
        """(N, N_prec, N * N_prec) of the task's last model update, [n*n][B] each"""
        out = [np.empty((self.dof * self.dof, self.B)) for _ in range(3)]
        self._rc(self.lib.sai2b_task_get_nullspaces(self.h, task, *[C.c_void_p(x.ctypes.data) for x in out]))
        return tuple(out)

    def get_mft_velocity(self, task):
        v, w = np.empty((3, self.B)), np.empty((3, self.B))
        self._rc(self.lib.sai2b_get_mft_velocity(self.h, task, C.c_void_p(v.ctypes.data), C.c_void_p(w.ctypes.data)))
        return v, w

    def get_mft_sigma(self, task):
        """sigmaForce, sigmaPosition, sigmaMoment, sigmaOrientation: [9][B] row-major each"""
        out = [np.empty((9, self.B)) for _ in range(4)]
        self._rc(self.lib.sai2b_get_mft_sigma(self.h, task, *[C.c_void_p(x.ctypes.data) for x in out]))
        return tuple(out)

    def set_mft_type1_posture(self, task, q_des):
        p, _ = self._in(q_des, self.dof)
        self._rc(self.lib.sai2b_set_mft_type1_posture(self.h, task, p, self._dev(q_des)))

    def get_singularity_types_count(self, task):
        """per robot: singular directions found by the last model update (SingularityHandler.h:211), no introspection needed"""
        n = np.empty(self.B, dtype=np.int32)
        self._rc(self.lib.sai2b_get_mft_singularity_state(self.h, task, C.c_void_p(n.ctypes.data), None, None))
        return n

    def get_mft_singularity_state(self, task):
        """per robot: singular directions of the last model update, type-1 and type-2 counts of the handler's history
        (SingularityHandler.h:211-215); no introspection needed"""
        n, c1, c2 = (np.empty(self.B, dtype=np.int32) for _ in range(3))
        self._rc(self.lib.sai2b_get_mft_singularity_state(self.h, task, *[C.c_void_p(x.ctypes.data) for x in (n, c1, c2)]))
        return n, c1, c2

    def synchronize(self):
        self._rc(self.lib.sai2b_synchronize(self.h))

    def stream(self):
        return self.lib.sai2b_stream(self.h)

    def device_buffer(self, which, task=-1):
        return self.lib.sai2b_device_buffer(self.h, which, task)

    def profile_tick(self, steps):
        """-> (first_kernel_ms, second_kernel_ms): HIP-event average duration per launch of each kernel of
        the fused tick, measured on the ctx stream"""
        a, b = C.c_double(), C.c_double()
        self._rc(self.lib.sai2b_profile_tick(self.h, int(steps), C.byref(a), C.byref(b)))
        return a.value, b.value

    def fallback_count(self):
        """robots of the last tick that ran the generic (Jacobi-SVD) kernel behind the SVD-free one"""
        n = C.c_int()
        self._rc(self.lib.sai2b_get_fallback_count(self.h, C.byref(n)))
        return n.value

    def worklist_state(self):
        """-> dict(last_seen, pending, form, wmax): the work list's length at the host's last look (that of the tick 8 before
        it; -1: none yet), how the request under way is answered (0: none, 1: mapped host words, 2: copies), what the last tick
        launched (0: the generic kernel alone, 1: an SVD-free kernel and the pass over its work list, 2: one launch, every
        wavefront serving the robots it declines) and the most robots one wavefront declined at that look (-1: not known)"""
        v = [C.c_int() for _ in range(4)]
        self._rc(self.lib.sai2b_get_worklist_state(self.h, *[C.byref(x) for x in v]))
        return {"last_seen": v[0].value, "pending": v[1].value, "form": v[2].value, "wmax": v[3].value}

    def counters(self):
        a, b = C.c_longlong(), C.c_longlong()
        self.lib.sai2b_counters(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    # -- introspection of the last tick
    def get_task_nullspace(self, task):
        out = np.empty((self.dof * self.dof, self.B))
        self._rc(self.lib.sai2b_get_task_nullspace(self.h, task, C.c_void_p(out.ctypes.data)))
        return out

    def get_task_torques(self, task):
        out = np.empty((self.dof, self.B))
        self._rc(self.lib.sai2b_get_task_torques(self.h, task, C.c_void_p(out.ctypes.data)))
        return out

    def get_mft_singularity(self, task):
        s, a, r = np.empty((6, self.B)), np.empty(self.B), np.empty(self.B)
        self._rc(self.lib.sai2b_get_mft_singularity(self.h, task, *[C.c_void_p(x.ctypes.data) for x in (s, a, r)]))
        return s, a, r

    def get_mft_task_forces(self, task):
        fu, ff = np.empty((6, self.B)), np.empty((6, self.B))
        self._rc(self.lib.sai2b_get_mft_task_forces(self.h, task, C.c_void_p(fu.ctypes.data), C.c_void_p(ff.ctypes.data)))
        return fu, ff

    def get_mft_status(self, task):
        """dict: pos [3,B], rot [9,B], sensed_force / sensed_moment (world frame) [3,B], pos_error, ori_error [3,B],
        pos_error_norm, ori_error_norm [B] (what goalPositionReached / goalOrientationReached compare)"""
        B = self.B
        names = ("pos", "rot", "sensed_force", "sensed_moment", "pos_error", "ori_error", "pos_error_norm", "ori_error_norm")
        out = [np.empty((r, B)) for r in (3, 9, 3, 3, 3, 3)] + [np.empty(B), np.empty(B)]
        self._rc(self.lib.sai2b_get_mft_status(self.h, task, *[C.c_void_p(x.ctypes.data) for x in out]))
        return dict(zip(names, out))

    def get_mft_goals(self, task):
        B = self.B
        out = [np.empty((r, B)) for r in (3, 9, 3, 3, 3, 3, 3, 3)]
        self._rc(self.lib.sai2b_get_mft_goals(self.h, task, *[C.c_void_p(x.ctypes.data) for x in out]))
        return tuple(out)

    def get_jt_goals(self, task):
        k0 = self.tasks[task].task_dof
        out = [np.empty((k0, self.B)) for _ in range(3)]
        self._rc(self.lib.sai2b_get_jt_goals(self.h, task, *[C.c_void_p(x.ctypes.data) for x in out]))
        return tuple(out)

    def reset_integrators(self, task, which=0):
        """0 all, 1 linear (position / force), 2 angular (orientation / moment); JointTask: all"""
        self._rc(self.lib.sai2b_reset_integrators(self.h, task, int(which)))

    # -- simulation harness
    def sim_step(self, tau=None, dt=0.001, substeps=1, with_gravity=False):
        """one control period of rigid-body dynamics under `tau` (None = the last computed torques; numpy
        [7][B] or a torch CUDA tensor), state updated in place on the device"""
        p, _ = self._in(tau, self.dof)
        self._rc(self.lib.sai2b_sim_step(self.h, p, self._dev(tau), float(dt), int(substeps), int(with_gravity)))

    def get_state(self):
        q, dq = np.empty((self.dof, self.B)), np.empty((self.dof, self.B))
        self._rc(self.lib.sai2b_get_state(self.h, C.c_void_p(q.ctypes.data), C.c_void_p(dq.ctypes.data)))
        return q, dq

    def get_bias(self, with_gravity=False):
        out = np.empty((self.dof, self.B))
        self._rc(self.lib.sai2b_get_bias(self.h, int(with_gravity), C.c_void_p(out.ctypes.data)))
        return out

    def get_jt_desired(self, task):
        """desired q, dq, ddq of a JointTask: the goal, or the internal OTG's next state"""
        k0 = self.tasks[task].task_dof
        out = [np.empty((k0, self.B)) for _ in range(3)]
        self._rc(self.lib.sai2b_get_jt_desired(self.h, task, *[C.c_void_p(x.ctypes.data) for x in out]))
        return tuple(out)

    def get_mft_desired(self, task):
        """desired position, orientation, linear/angular velocity, linear/angular acceleration"""
        B = self.B
        out = [np.empty((r, B)) for r in (3, 9, 3, 3, 3, 3)]
        self._rc(self.lib.sai2b_get_mft_desired(self.h, task, *[C.c_void_p(x.ctypes.data) for x in out]))
        return tuple(out)

    def get_otg_status(self, task):
        """per robot: isGoalReached() and the last ruckig Result of the task's internal OTG"""
        a, b = np.empty(self.B), np.empty(self.B)
        self._rc(self.lib.sai2b_get_otg_status(self.h, task, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data)))
        return a, b

    def get_model(self, task=-1):
        M = np.empty((self.dof * self.dof, self.B))
        if task < 0:
            self._rc(self.lib.sai2b_get_model(self.h, -1, C.c_void_p(M.ctypes.data), None, None, None))
            return M
        J, x, R = np.empty((6 * self.dof, self.B)), np.empty((3, self.B)), np.empty((9, self.B))
        self._rc(self.lib.sai2b_get_model(self.h, task, *[C.c_void_p(a.ctypes.data) for a in (M, J, x, R)]))
        return M, J, x, R


# --------------------------------------------------------------------------------------------------
# reference-named, batch-aware facade
# --------------------------------------------------------------------------------------------------
class SnapshotBank:
    """sai2b_snapshot_bank: `capacity` slots of whole robot states on the device (sai2b.h "snapshot banks"). save / load move
    robot b with mask[b] != 0 (None: every robot) to / from slot slots[b] (None: slot b); slots and mask are numpy arrays or
    torch CUDA tensors (int32 / bool or uint8; then nothing leaves the device and nothing synchronises). A robot whose slot
    is out of range, or on load was never saved, is left alone and counted. Close the bank before its controller."""

    def __init__(self, ctrl, capacity, what=_abi.SNAP_EPISODE):
        self._ctrl, self.lib = ctrl, ctrl.lib
        self.capacity, self.what = int(capacity), int(what)
        h = C.c_void_p()
        ctrl._rc(self.lib.sai2b_snapshot_bank_create(ctrl.h, self.capacity, self.what, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.sai2b_snapshot_bank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _move(self, fn, slots, mask):
        c = self._ctrl
        dev = c._dev(slots, mask)
        ps, ks = c._slots(slots) if slots is not None else (None, None)
        pm, km = c._mask(mask) if mask is not None else (None, None)
        c._rc(fn(c.h, self.h, ps, pm, dev))

    def save(self, slots=None, mask=None):
        self._move(self.lib.sai2b_snapshot_save, slots, mask)

    def load(self, slots=None, mask=None):
        self._move(self.lib.sai2b_snapshot_load, slots, mask)

    def counts(self):
        """of the controller's last save() / load(): dict 'moved', 'out_of_range', 'never_saved' -> robots"""
        c = (C.c_int * 3)()
        self._ctrl._rc(self.lib.sai2b_get_snapshot_counts(self._ctrl.h, c))
        return dict(zip(_abi.SNAP_COUNTS, list(c)))

    def export_size(self):
        return int(self.lib.sai2b_snapshot_export_size(self.h))

    def export(self):
        """the bank as a numpy uint8 blob: header, words, valid bytes"""
        blob = np.empty(self.export_size(), dtype=np.uint8)
        _check(self.lib, None, self.lib.sai2b_snapshot_export(self.h, C.c_void_p(blob.ctypes.data), blob.size))
        return blob

    def import_(self, blob):
        """a blob of export() into this bank; ValueError (naming the first differing block) when its layout is not the bank's"""
        arr = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        _check(self.lib, None, self.lib.sai2b_snapshot_import(self.h, C.c_void_p(arr.ctypes.data), arr.size))


class BatchedRobotModel:
    """Stands where the reference takes ``std::shared_ptr<Sai2Model::Sai2Model>``: the constant
    model plus the batch size and the device; q/dq are set on it as on the reference's model
    (examples/05-using_robot_controller.cpp:143-145)."""

    def __init__(self, batch, model=None, device=0, urdf_file=None):
        self.batch = int(batch)
        self.device = int(device)
        self.links = None
        if urdf_file is not None:  # Sai2Model::Sai2Model(urdf_file) (examples/05-...cpp:96-97)
            model, self.links = model_from_urdf(urdf_file)
        self.model = model if model is not None else panda_model()
        self._q = np.zeros((self.model.dof, self.batch))
        self._dq = np.zeros((self.model.dof, self.batch))
        self._controller = None
        self._standalone = []  # tasks driven on their own (TemplateTask-level calls): each has its 1-task context
        self._payloads = {}  # 'controller' / 'plant' -> (link, mass, com, inertia): applied to contexts created later too

    def dof(self):
        return int(self.model.dof)

    def setTRobotBase(self, pos, rot=None):
        """Sai2Model::setTRobotBase (examples/05-using_robot_controller.cpp:69): the robot base in the world; replaces an
        earlier one. Part of the model the kernels see (with_base_transform): before a controller or a task runs on it."""
        if self._controller is not None or self._standalone:
            raise ValueError("setTRobotBase must be called before a controller or a task runs on this robot model")
        if not hasattr(self, "_model_in_base"):
            self._model_in_base = self.model
        self.model = with_base_transform(self._model_in_base, pos, rot)
        self._base = (np.array(pos, dtype=np.float64).reshape(3), np.eye(3) if rot is None else np.array(rot, dtype=np.float64).reshape(3, 3))

    def TRobotBase(self):
        """(position, rotation) of the base in the world"""
        return getattr(self, "_base", (np.zeros(3), np.eye(3)))

    def setQ(self, q):
        self._q = q
        self._push()

    def setDq(self, dq):
        self._dq = dq
        self._push()

    def q(self):
        return self._q

    def dq(self):
        return self._dq

    def updateModel(self):
        """kept for call-order compatibility: the model update is fused into the tick kernel"""
        self._push()

    def _push(self):
        if self._controller is not None:
            self._controller._ctrl.set_state(self._q, self._dq)
        for own in self._standalone:
            own._ctrl.set_state(self._q, self._dq)

    def setLinkPayload(self, link, mass, com=None, inertia=None, target="both"):
        """What each robot of the batch carries: one rigid body on `link` (0-based moving link, or a URDF link name when the
        model came from a URDF file), per robot mass [B], com [3][B] in that link's frame, inertia [6][B] about the body's
        COM. Where the reference gives each robot its own Sai2Model, the batch shares one model and differs in these rows
        (Controller.set_link_payload). Kept for controllers and tasks created on this model later."""
        if isinstance(link, str):
            if self.links is None:
                raise ValueError("setLinkPayload: a link name needs a model read from a URDF file")
            idx, pos, R = resolve_link_frame(self.links, link)
            if not (np.allclose(pos, 0) and np.allclose(R, np.eye(3))):  # a fixed-joint child: re-express in the moving link
                if hasattr(mass, "data_ptr"):
                    raise ValueError("setLinkPayload: a payload on a fixed-joint link takes host arrays")
                B = self.batch
                c = np.zeros((3, B)) if com is None else np.asarray(com, dtype=np.float64)
                com = pos[:, None] + R @ c
                if inertia is not None:
                    i6 = np.asarray(inertia, dtype=np.float64)
                    I = np.stack([i6[[0, 3, 4]], i6[[3, 1, 5]], i6[[4, 5, 2]]])  # [3][3][B]
                    I = np.einsum("ij,jkb,lk->ilb", R, I, R)
                    inertia = np.stack([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]])
            link = idx
        if target not in _abi.PAYLOAD_TARGETS:
            raise ValueError("target must be 'controller', 'plant' or 'both'")
        for name in (("controller", "plant") if target == "both" else (target,)):
            self._payloads[name] = (int(link), mass, com, inertia)
        for c in self._contexts():
            c.set_link_payload(int(link), mass, com, inertia, target)

    def clearLinkPayload(self, target="both"):
        if target not in _abi.PAYLOAD_TARGETS:
            raise ValueError("target must be 'controller', 'plant' or 'both'")
        for name in (("controller", "plant") if target == "both" else (target,)):
            self._payloads.pop(name, None)
        for c in self._contexts():
            c.clear_link_payload(target)

    def _contexts(self):
        return ([self._controller._ctrl] if self._controller is not None else []) + [own._ctrl for own in self._standalone]

    def _apply_payloads(self, ctrl):
        for name, (link, mass, com, inertia) in self._payloads.items():
            ctrl.set_link_payload(link, mass, com, inertia, name)


class _StandaloneOwner:
    """What a task that is not attached to a RobotController runs on: a context holding that one task
    (sai2b.h "task-level plugin interface"). Created on the first call that needs the device."""

    def __init__(self, robot, cfg, q_construction):
        self._ctrl = Controller(robot.model, [cfg], robot.batch, robot.device)
        robot._apply_payloads(self._ctrl)
        # the reference constructs a task at the model's state of that moment (goals := current pose)
        self._ctrl.set_state(q_construction, np.zeros_like(q_construction))
        self._ctrl.reinitialize()
        self._ctrl.set_state(robot.q(), robot.dq())
        robot._standalone.append(self)


class _InternalOtgView:
    """read-only side of the task's OTG_joints / OTG_6dof_cartesian object (JointTask.h:324 `getInternalOtg()`,
    OTG_joints.h:110-164, OTG_6dof_cartesian.h:171-243): one answer per robot"""

    def __init__(self, task):
        self._t = task

    def isGoalReached(self):
        rc, idx = self._t._require_owner()
        return rc._ctrl.get_otg_status(idx)[0] != 0

    def getJerkLimitEnabled(self):
        return bool(self._t._cfg.use_internal_otg and self._t._cfg.internal_otg_jerk_limited)

    def getNextPosition(self):
        return self._t.getDesiredPosition()

    def getNextVelocity(self):
        return self._t.getDesiredVelocity()

    def getNextAcceleration(self):
        return self._t.getDesiredAcceleration()

    def getNextOrientation(self):
        return self._t.getDesiredOrientation()

    def getNextLinearVelocity(self):
        return self._t.getDesiredLinearVelocity()

    def getNextAngularVelocity(self):
        return self._t.getDesiredAngularVelocity()

    def getNextLinearAcceleration(self):
        return self._t.getDesiredLinearAcceleration()

    def getNextAngularAcceleration(self):
        return self._t.getDesiredAngularAcceleration()


class _TaskBase:
    def __init__(self, robot, cfg):
        self._robot = robot
        self._cfg = cfg
        self._owner = None  # (RobotController, index) once attached; (_StandaloneOwner, 0) when driven on its own
        self._pending = {}
        self._q_construction = np.array(robot.q(), dtype=np.float64, copy=True) if not hasattr(robot.q(), "data_ptr") else robot.q().cpu().numpy()
        self._task_level = False  # the last model update came through updateTaskModel()

    # TemplateTask accessors (reference src/tasks/TemplateTask.h:95-115)
    def getInternalOtg(self):
        return _InternalOtgView(self)

    def getTaskName(self):
        return self._cfg.name.decode()

    def getTaskType(self):
        return self._cfg.type

    def getLoopTimestep(self):
        return self._cfg.loop_timestep

    def getConstRobotModel(self):
        return self._robot

    def setDynamicDecouplingType(self, t):
        self._cfg.dynamic_decoupling_type = int(t)
        self._sync_cfg()

    def setBoundedInertiaEstimateThreshold(self, thr):
        self._cfg.bie_threshold = max(float(thr), 0.0)  # JointTask.h:369-375
        self._sync_cfg()

    def _sync_cfg(self):
        if self._owner:
            rc, idx = self._owner
            rc._ctrl.update_task_config(idx, self._cfg)

    def _goal(self, key, value, rows):
        B = self._robot.batch
        if not hasattr(value, "data_ptr"):
            value = np.ascontiguousarray(value, dtype=np.float64)
            if value.shape != (rows, B):
                raise ValueError(f"goal must have shape ({rows}, {B})")
        self._pending[key] = value
        self._flush()

    # ---- the TemplateTask virtuals (reference src/tasks/TemplateTask.h:42-88): a task driven on its own, the
    # caller chaining the nullspaces as in examples/04-task_and_redundancy.cpp:141-150,188-189
    def updateTaskModel(self, N_prec=None):
        """N_prec [n*n][B] (row-major inside the component index), None = identity"""
        rc, idx = self._require_owner()
        rc._ctrl.task_update_model(idx, N_prec)
        self._task_level = True

    def computeTorques(self, tau_prec=None, out=None):
        """computeTorques() / computeTorques(tau_prec): this task's torques [n][B]"""
        rc, idx = self._require_owner()
        return rc._ctrl.task_compute_torques(idx, tau_prec, out)

    def reInitializeTask(self, mask=None):
        """mask [B] (bool / uint8): only for the robots it selects"""
        rc, idx = self._require_owner()
        if mask is None:
            rc._ctrl.task_reinitialize(idx)
        else:
            rc._ctrl.reinitialize_robots(mask, idx)

    def getTaskNullspace(self):
        rc, idx = self._require_owner()
        return rc._ctrl.task_nullspaces(idx)[0]

    def getPreviousTasksNullspace(self):
        rc, idx = self._require_owner()
        return rc._ctrl.task_nullspaces(idx)[1]

    def getTaskAndPreviousNullspace(self):
        rc, idx = self._require_owner()
        if self._task_level:
            return rc._ctrl.task_nullspaces(idx)[2]
        return rc._ctrl.get_task_nullspace(idx)  # of the controller's last tick (introspection on)

    def _require_owner(self):
        if not self._owner:
            self._owner = (_StandaloneOwner(self._robot, self._cfg, self._q_construction), 0)
            self._flush()
        return self._owner


class JointTask(_TaskBase):
    """reference src/tasks/JointTask.h:56-75 (ctors), :137-179 (goals), :234-259 (gains)"""

    def __init__(self, robot, joint_selection_matrix=None, task_name="joint_task", loop_timestep=0.001):
        cfg = joint_task_config(task_name, joint_selection_matrix, internal_otg=True, robot_dof=robot.dof())  # JointTask.h:38
        cfg.loop_timestep = loop_timestep
        super().__init__(robot, cfg)

    def isFullJointTask(self):
        return self._cfg.task_dof == self._robot.dof()

    def setGoalPosition(self, q):
        self._goal("q", q, self._cfg.task_dof)

    def setGoalVelocity(self, dq):
        self._goal("dq", dq, self._cfg.task_dof)

    def setGoalAcceleration(self, ddq):
        self._goal("ddq", ddq, self._cfg.task_dof)

    def setGains(self, kp, kv, ki=0.0, _checked=True):
        """JointTask.h:225-257 (JointTask.cpp:136-205): scalars / size-1 vectors = isotropic, else one gain per task
        coordinate; vectors are rejected only when every entry is negative (JointTask.cpp:171)"""
        k0 = self._cfg.task_dof
        a = [np.atleast_1d(np.asarray(x, dtype=float)) for x in (kp, kv, ki)]
        iso = all(x.size == 1 for x in a)
        if not iso:
            a[2] = np.zeros(k0) if np.ndim(ki) == 0 and ki == 0.0 else a[2]  # the two-vector overload: ki = 0
            if any(x.size != k0 for x in a):
                raise ValueError("size of gain vectors inconsistent with number of task dofs in JointTask::setGains\n")
        if _checked and (any(x[0] < 0 for x in a) if iso else any(x.max() < 0 for x in a)):
            raise ValueError("gains must be positive or zero in JointTask::setGains\n")
        kp, kv, ki = (np.broadcast_to(x, (k0,)) for x in a)
        for i in range(k0):
            self._cfg.kp[i], self._cfg.kv[i], self._cfg.ki[i] = kp[i], kv[i], ki[i]
        if not _checked:
            self._cfg.unsafe_motion_gains = 1
        self._sync_cfg()

    def setGainsUnsafe(self, kp, kv, ki):
        """JointTask.h:256: no sign check"""
        self.setGains(kp, kv, ki, _checked=False)

    def getJointSelectionMatrix(self):
        """JointTask.h:120: [task_dof, dof]"""
        n = self._robot.dof()
        return np.array(self._cfg.joint_selection[: self._cfg.task_dof * n]).reshape(self._cfg.task_dof, n)

    def getVelocitySaturationMaxVelocity(self):
        """JointTask.h:352"""
        return np.array(self._cfg.saturation_velocity[: self._cfg.task_dof])

    def enableVelocitySaturation(self, saturation_velocity):
        v = np.broadcast_to(np.asarray(saturation_velocity, dtype=float), (self._cfg.task_dof,))
        if v.min() <= 0:
            raise ValueError("saturation velocity must be positive in JointTask::enableVelocitySaturation\n")
        self._cfg.use_velocity_saturation = 1
        for i in range(self._cfg.task_dof):
            self._cfg.saturation_velocity[i] = v[i]
        self._sync_cfg()

    def disableVelocitySaturation(self):
        self._cfg.use_velocity_saturation = 0
        self._sync_cfg()

    def getGoalPosition(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_jt_goals(idx)[0]

    def getGoalVelocity(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_jt_goals(idx)[1]

    def getGoalAcceleration(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_jt_goals(idx)[2]

    def getCurrentPosition(self):
        """S q (JointTask.h:130), from the controller's state buffer"""
        rc, idx = self._require_owner()
        S = np.array(self._cfg.joint_selection[: self._cfg.task_dof * self._robot.dof()]).reshape(self._cfg.task_dof, self._robot.dof())
        return S @ rc._ctrl.get_state()[0]

    def getCurrentVelocity(self):
        rc, idx = self._require_owner()
        S = np.array(self._cfg.joint_selection[: self._cfg.task_dof * self._robot.dof()]).reshape(self._cfg.task_dof, self._robot.dof())
        return S @ rc._ctrl.get_state()[1]

    def getGains(self):
        """one (kp, kv, ki) when the gains are isotropic, one per task coordinate otherwise (JointTask.cpp:207-216)"""
        k0 = self._cfg.task_dof
        g = [(self._cfg.kp[i], self._cfg.kv[i], self._cfg.ki[i]) for i in range(k0)]
        return g[:1] if all(x == g[0] for x in g) else g

    def getTaskDof(self):
        return self._cfg.task_dof

    def getVelocitySaturationEnabled(self):
        return bool(self._cfg.use_velocity_saturation)

    def getBoundedInertiaEstimateThreshold(self):
        return self._cfg.bie_threshold

    def resetIntegrators(self):
        rc, idx = self._require_owner()
        rc._ctrl.reset_integrators(idx)

    def enableInternalOtgAccelerationLimited(self, max_velocity, max_acceleration):
        """JointTask.cpp:360-381 (scalars or per-task-dof vectors)"""
        k0 = self._cfg.task_dof
        v, a = (np.broadcast_to(np.asarray(x, dtype=float), (k0,)) for x in (max_velocity, max_acceleration))
        if v.min() <= 0:
            raise ValueError("max velocity cannot be 0 or negative in any directions in OTG_joints::setMaxVelocity\n")
        if a.min() <= 0:
            raise ValueError("max acceleration cannot be 0 or negative in any directions in OTG_joints::setMaxAcceleration\n")
        for i in range(k0):
            self._cfg.otg_max_velocity[i], self._cfg.otg_max_acceleration[i] = v[i], a[i]
        self._cfg.use_internal_otg, self._cfg.internal_otg_jerk_limited = 1, 0
        self._sync_cfg()

    def enableInternalOtgJerkLimited(self, max_velocity, max_acceleration, max_jerk):
        """JointTask.cpp:383-406 (scalars or per-task-dof vectors): ruckig's jerk-limited interface"""
        k0 = self._cfg.task_dof
        v, a, j = (np.broadcast_to(np.asarray(x, dtype=float), (k0,)) for x in (max_velocity, max_acceleration, max_jerk))
        if v.min() <= 0:
            raise ValueError("max velocity cannot be 0 or negative in any directions in OTG_joints::setMaxVelocity\n")
        if a.min() <= 0:
            raise ValueError("max acceleration cannot be 0 or negative in any directions in OTG_joints::setMaxAcceleration\n")
        if j.min() <= 0:
            raise ValueError("max jerk cannot be 0 or negative in any directions in OTG_joints::setMaxJerk\n")
        for i in range(k0):
            self._cfg.otg_max_velocity[i], self._cfg.otg_max_acceleration[i], self._cfg.otg_max_jerk[i] = v[i], a[i], j[i]
        self._cfg.use_internal_otg, self._cfg.internal_otg_jerk_limited = 1, 1
        self._sync_cfg()

    def disableInternalOtg(self):
        """JointTask.h:320: desired state = goal state"""
        self._cfg.use_internal_otg = 0
        self._sync_cfg()

    def getInternalOtgEnabled(self):
        return bool(self._cfg.use_internal_otg)

    def getDesiredPosition(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_jt_desired(idx)[0]

    def getDesiredVelocity(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_jt_desired(idx)[1]

    def getDesiredAcceleration(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_jt_desired(idx)[2]

    def _flush(self):
        if self._owner and self._pending:
            rc, idx = self._owner
            rc._ctrl.set_jt_goals(idx, self._pending.get("q"), self._pending.get("dq"), self._pending.get("ddq"))
            self._pending = {}


class MotionForceTask(_TaskBase):
    """reference src/tasks/MotionForceTask.h:96-110 (ctors), :211-247 (goals), :272-328 (gains),
    :576-623 (force space)"""

    def __init__(self, robot, link=EE_LINK, compliant_frame_pos=EE_FRAME_POS, compliant_frame_rot=None,
                 controlled_directions_translation=None, controlled_directions_rotation=None,
                 task_name=None, is_force_motion_parametrization_in_compliant_frame=False, loop_timestep=0.001):
        partial = None
        if controlled_directions_translation is not None or controlled_directions_rotation is not None:
            partial = (
                np.zeros((0, 3)) if controlled_directions_translation is None else controlled_directions_translation,
                np.zeros((0, 3)) if controlled_directions_rotation is None else controlled_directions_rotation,
            )
        if isinstance(link, str):  # a link NAME as in the reference: needs a robot built from a URDF file
            if robot.links is None:
                raise ValueError("link names need a robot model built from a URDF file")
            link, compliant_frame_pos, compliant_frame_rot = resolve_link_frame(robot.links, link, compliant_frame_pos, compliant_frame_rot)
        cfg = motion_force_task_config(task_name, link, compliant_frame_pos, compliant_frame_rot, partial,
                                       internal_otg=True, robot_dof=robot.dof())  # MotionForceTask.h:67
        cfg.parametrization_in_compliant_frame = int(is_force_motion_parametrization_in_compliant_frame)
        cfg.loop_timestep = loop_timestep
        super().__init__(robot, cfg)

    def setGoalPosition(self, x):
        self._goal("pos", x, 3)

    def setGoalOrientation(self, R):
        self._goal("rot", R, 9)

    def setGoalLinearVelocity(self, v):
        self._goal("v", v, 3)

    def setGoalAngularVelocity(self, w):
        self._goal("w", w, 3)

    def setGoalLinearAcceleration(self, a):
        self._goal("a", a, 3)

    def setGoalAngularAcceleration(self, a):
        self._goal("alpha", a, 3)

    def setGoalForce(self, f):
        self._goal("f", f, 3)

    def setGoalMoment(self, m):
        self._goal("m", m, 3)

    def updateSensedForceAndMoment(self, f, m):
        self._goal("sf", f, 3)
        self._goal("sm", m, 3)
        self._sensed_sensor = (f, m)

    def getSensedForceSensor(self):
        """MotionForceTask.h:173,183: the last sensor-frame readings handed to updateSensedForceAndMoment"""
        return getattr(self, "_sensed_sensor", (np.zeros((3, self._robot.batch)),) * 2)[0]

    def getSensedMomentSensor(self):
        return getattr(self, "_sensed_sensor", (np.zeros((3, self._robot.batch)),) * 2)[1]

    def _set3(self, names, values, where):
        vals = [np.broadcast_to(np.asarray(v, dtype=float), (3,)) for v in values]
        if min(v.min() for v in vals) < 0:
            raise ValueError(f"all gains should be positive or zero in MotionForceTask::{where}\n")
        for n, v in zip(names, vals):
            for i in range(3):
                getattr(self._cfg, n)[i] = v[i]
        self._sync_cfg()

    def setPosControlGains(self, kp, kv, ki=0.0):
        self._set3(("kp_pos", "kv_pos", "ki_pos"), (kp, kv, ki), "setPosControlGains")

    def setOriControlGains(self, kp, kv, ki=0.0):
        self._set3(("kp_ori", "kv_ori", "ki_ori"), (kp, kv, ki), "setOriControlGains")

    def setForceControlGains(self, kp, kv, ki):
        self._set3(("kp_force", "kv_force", "ki_force"), (kp, kv, ki), "setForceControlGains")

    def setMomentControlGains(self, kp, kv, ki):
        self._set3(("kp_moment", "kv_moment", "ki_moment"), (kp, kv, ki), "setMomentControlGains")

    def _parametrize(self, dim_field, axis_field, dim, axis, dim_msg, axis_msg):
        """-> whether the space changed (`reset` of MotionForceTask.cpp:838-848); the library then moves that half of
        the goal to the current pose, restarts that half of the internal OTG there and resets its integrators"""
        if not 0 <= dim <= 3:
            raise ValueError(dim_msg)
        old_dim, old_axis = getattr(self._cfg, dim_field), np.array(getattr(self._cfg, axis_field)[:])
        if dim in (1, 2):
            a = np.asarray(axis, dtype=float)
            if np.linalg.norm(a) < 1e-2:
                raise ValueError(axis_msg)
            a = a / np.linalg.norm(a)
            for i in range(3):
                getattr(self._cfg, axis_field)[i] = a[i]
        setattr(self._cfg, dim_field, int(dim))
        self._sync_cfg()
        if dim != old_dim:
            return True
        if dim not in (1, 2):
            return False
        new_axis = np.array(getattr(self._cfg, axis_field)[:])
        return not (np.sum((new_axis - old_axis) ** 2) <= 1e-24 * min(np.sum(new_axis ** 2), np.sum(old_axis ** 2)))

    def parametrizeForceMotionSpaces(self, force_space_dimension, axis=(0, 0, 1)):
        return self._parametrize("force_space_dimension", "force_axis", force_space_dimension, axis,
                                 "Force space dimension should be between 0 and 3 in MotionForceTask::parametrizeForceMotionSpaces\n",
                                 "Force or motion axis should be a non singular vector in MotionForceTask::parametrizeForceMotionSpaces\n")

    def parametrizeMomentRotMotionSpaces(self, moment_space_dimension, axis=(0, 0, 1)):
        return self._parametrize("moment_space_dimension", "moment_axis", moment_space_dimension, axis,
                                 "Moment space dimension should be between 0 and 3 in MotionForceTask::parametrizeMomentRotMotionSpaces\n",
                                 "Moment or rot motion axis should be a non singular vector in MotionForceTask::parametrizeMomentRotMotionSpaces\n")

    def setClosedLoopForceControl(self, on=True):
        self._cfg.closed_loop_force = int(on)
        self._sync_cfg()

    def enablePassivity(self):
        self._cfg.passivity_enabled = 1
        self._sync_cfg()

    def disablePassivity(self):
        self._cfg.passivity_enabled = 0
        self._sync_cfg()

    def setClosedLoopMomentControl(self, on=True):
        self._cfg.closed_loop_moment = int(on)
        self._sync_cfg()

    def enableVelocitySaturation(self, linear_vel_sat=0.3, angular_vel_sat=np.pi / 3):
        if linear_vel_sat <= 0 or angular_vel_sat <= 0:
            raise ValueError("Velocity saturation values should be strictly positive or zero in MotionForceTask::enableVelocitySaturation\n")
        self._cfg.use_velocity_saturation = 1
        self._cfg.linear_saturation_velocity, self._cfg.angular_saturation_velocity = linear_vel_sat, angular_vel_sat
        self._sync_cfg()

    def disableVelocitySaturation(self):
        self._cfg.use_velocity_saturation = 0
        self._sync_cfg()

    def enableInternalOtgAccelerationLimited(self, max_linear_velocity, max_linear_acceleration, max_angular_velocity,
                                             max_angular_acceleration):
        """MotionForceTask.cpp:511-523"""
        c = self._cfg
        if min(max_linear_velocity, max_angular_velocity) <= 0:
            raise ValueError("max velocity set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxLinearVelocity\n")
        if min(max_linear_acceleration, max_angular_acceleration) <= 0:
            raise ValueError("max acceleration set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxLinearAcceleration\n")
        c.otg_max_linear_velocity, c.otg_max_linear_acceleration = float(max_linear_velocity), float(max_linear_acceleration)
        c.otg_max_angular_velocity, c.otg_max_angular_acceleration = float(max_angular_velocity), float(max_angular_acceleration)
        c.use_internal_otg, c.internal_otg_jerk_limited = 1, 0
        self._sync_cfg()

    def enableInternalOtgJerkLimited(self, max_linear_velocity, max_linear_acceleration, max_linear_jerk, max_angular_velocity,
                                     max_angular_acceleration, max_angular_jerk):
        """MotionForceTask.cpp:525-538: ruckig's jerk-limited interface"""
        c = self._cfg
        if min(max_linear_velocity, max_angular_velocity) <= 0:
            raise ValueError("max velocity set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxLinearVelocity\n")
        if min(max_linear_acceleration, max_angular_acceleration) <= 0:
            raise ValueError("max acceleration set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxLinearAcceleration\n")
        if min(max_linear_jerk, max_angular_jerk) <= 0:
            raise ValueError("max jerk set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxJerk\n")
        c.otg_max_linear_velocity, c.otg_max_linear_acceleration = float(max_linear_velocity), float(max_linear_acceleration)
        c.otg_max_angular_velocity, c.otg_max_angular_acceleration = float(max_angular_velocity), float(max_angular_acceleration)
        c.otg_max_linear_jerk, c.otg_max_angular_jerk = float(max_linear_jerk), float(max_angular_jerk)
        c.use_internal_otg, c.internal_otg_jerk_limited = 1, 1
        self._sync_cfg()

    def disableInternalOtg(self):
        """MotionForceTask.h:423: desired state = goal state"""
        self._cfg.use_internal_otg = 0
        self._sync_cfg()

    def getInternalOtgEnabled(self):
        return bool(self._cfg.use_internal_otg)

    def getDesiredPosition(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_desired(idx)[0]

    def getDesiredOrientation(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_desired(idx)[1]

    def getDesiredLinearVelocity(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_desired(idx)[2]

    def getDesiredAngularVelocity(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_desired(idx)[3]

    def getDesiredLinearAcceleration(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_desired(idx)[4]

    def getDesiredAngularAcceleration(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_desired(idx)[5]

    def setSingularityHandlingBounds(self, s_min, s_max):
        self._cfg.s_min, self._cfg.s_max = float(s_min), float(s_max)
        self._sync_cfg()

    def _status(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_status(idx)

    def getCurrentPosition(self):
        return self._status()["pos"]

    def getCurrentOrientation(self):
        return self._status()["rot"]

    def getSensedForceControlWorldFrame(self):
        return self._status()["sensed_force"]

    def getSensedMomentControlWorldFrame(self):
        return self._status()["sensed_moment"]

    def getPositionError(self):
        return self._status()["pos_error"]

    def getOrientationError(self):
        return self._status()["ori_error"]

    def goalPositionReached(self, tolerance):
        """per robot (MotionForceTask.cpp:548-563)"""
        return self._status()["pos_error_norm"] < tolerance

    def goalOrientationReached(self, tolerance):
        return self._status()["ori_error_norm"] < tolerance

    def getGoalPosition(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_goals(idx)[0]

    def getGoalOrientation(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_goals(idx)[1]

    def _world_wrench(self, which):
        """MotionForceTask.cpp:755-769: a goal given in the compliant frame comes back in the WORLD frame"""
        rc, idx = self._require_owner()
        g = rc._ctrl.get_mft_goals(idx)[which]
        if not self._cfg.parametrization_in_compliant_frame:
            return g
        R = self._status()["rot"].T.reshape(-1, 3, 3)
        return np.ascontiguousarray(np.einsum("bij,jb->ib", R, g))

    def getGoalForce(self):
        return self._world_wrench(6)

    def getGoalMoment(self):
        return self._world_wrench(7)

    def getGoalLinearVelocity(self):
        """MotionForceTask.h:224-247"""
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_goals(idx)[2]

    def getGoalAngularVelocity(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_goals(idx)[3]

    def getGoalLinearAcceleration(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_goals(idx)[4]

    def getGoalAngularAcceleration(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_goals(idx)[5]

    def getLinearSaturationVelocity(self):
        """MotionForceTask.h:437-440"""
        return self._cfg.linear_saturation_velocity

    def getAngularSaturationVelocity(self):
        return self._cfg.angular_saturation_velocity

    def posSelectionProjector(self):
        """MotionForceTask.h:653-659: 3 x 3 diagonal blocks of the partial-task projection"""
        return np.array(self._cfg.partial_projection[:]).reshape(6, 6)[:3, :3].copy()

    def oriSelectionProjector(self):
        return np.array(self._cfg.partial_projection[:]).reshape(6, 6)[3:, 3:].copy()

    def setSingularityHandlingGains(self, kp_type_1, kv_type_1, kv_type_2):
        """MotionForceTask.h:748-753"""
        self._cfg.kp_type_1, self._cfg.kv_type_1, self._cfg.kv_type_2 = float(kp_type_1), float(kv_type_1), float(kv_type_2)
        self._sync_cfg()

    def enableSingularityHandling(self):
        self._cfg.enforce_handling_strategy = 1
        self._sync_cfg()

    def disableSingularityHandling(self):
        self._cfg.enforce_handling_strategy = 0
        self._sync_cfg()

    def setSingularVectorSign(self, convention):
        """Not in the reference: which way classifySingularity perturbs along a singular vector
        (SingularityHandler.cpp:253-265 uses V_s as Eigen's JacobiSVD left it, a sign Eigen does not specify).
        0 = largest-magnitude component of V_s[:, i] positive (default), 1 = the opposite, 2 = type 1 if either
        direction moves the task, 3 = only if both do (enum sai2b_singular_vector_sign)."""
        self._cfg.singular_vector_sign = int(convention)
        self._sync_cfg()

    def setFeedforwardForceGain(self, kff):
        self._cfg.kff_force = float(kff)
        self._sync_cfg()

    def getFeedforwardForceGain(self):
        return self._cfg.kff_force

    def setFeedforwardmomentGain(self, kff):
        self._cfg.kff_moment = float(kff)
        self._sync_cfg()

    def getFeedforwardmomentGain(self):
        return self._cfg.kff_moment

    def setMaxForceControlFeedbackOutput(self, v):
        self._cfg.max_force_feedback = float(v)
        self._sync_cfg()

    def getMaxForceControlFeedbackOutput(self):
        return self._cfg.max_force_feedback

    def setMaxMomentControlFeedbackOutput(self, v):
        self._cfg.max_moment_feedback = float(v)
        self._sync_cfg()

    def getMaxMomentControlFeedbackOutput(self):
        return self._cfg.max_moment_feedback

    def setForceSensorFrame(self, *args):
        """MotionForceTask::setForceSensorFrame (MotionForceTask.cpp:794-803). Two forms:
        (link, sensor_pos_in_link, sensor_rot_in_link=None) — the reference's: link index or NAME, the sensor frame in
        that link, which must be the control frame's; _T_control_to_sensor = compliant_frame^-1 * transformation_in_link;
        (sensor_pos_in_control_frame, sensor_rot_in_control_frame=None) — _T_control_to_sensor given directly."""
        if isinstance(args[0], (int, np.integer, str)):
            link, ps = args[0], np.asarray(args[1], dtype=float)
            Rs = np.eye(3) if len(args) < 3 or args[2] is None else np.asarray(args[2], dtype=float).reshape(3, 3)
            if isinstance(link, str):
                if self._robot.links is None:
                    raise ValueError("link names need a robot model built from a URDF file")
                link, ps, Rs = resolve_link_frame(self._robot.links, link, ps, Rs)
            if int(link) != self._cfg.link:
                raise ValueError("The link to which is attached the sensor should be the same as the link to which is attached "
                                 "the control frame in MotionForceTask::setForceSensorFrame\n")
            Rc, pc = np.array(self._cfg.frame_rot[:]).reshape(3, 3), np.array(self._cfg.frame_pos[:])
            return self.setForceSensorFrame(Rc.T @ (np.asarray(ps) - pc), Rc.T @ Rs)
        sensor_pos_in_control_frame = args[0]
        sensor_rot_in_control_frame = args[1] if len(args) > 1 else None
        p = np.asarray(sensor_pos_in_control_frame, dtype=float)
        R = np.eye(3) if sensor_rot_in_control_frame is None else np.asarray(sensor_rot_in_control_frame, dtype=float)
        for i in range(3):
            self._cfg.sensor_pos[i] = p[i]
        for i in range(9):
            self._cfg.sensor_rot[i] = R.ravel()[i]
        self._sync_cfg()

    def getForceSpaceDimension(self):
        return self._cfg.force_space_dimension

    def getMomentSpaceDimension(self):
        return self._cfg.moment_space_dimension

    def getPosControlGains(self):
        return [(self._cfg.kp_pos[i], self._cfg.kv_pos[i], self._cfg.ki_pos[i]) for i in range(3)]

    def getOriControlGains(self):
        return [(self._cfg.kp_ori[i], self._cfg.kv_ori[i], self._cfg.ki_ori[i]) for i in range(3)]

    def getVelocitySaturationEnabled(self):
        return bool(self._cfg.use_velocity_saturation)

    def getBoundedInertiaEstimateThreshold(self):
        return self._cfg.bie_threshold

    def resetIntegrators(self):
        rc, idx = self._require_owner()
        rc._ctrl.reset_integrators(idx, 0)

    def resetIntegratorsLinear(self):
        rc, idx = self._require_owner()
        rc._ctrl.reset_integrators(idx, 1)

    def resetIntegratorsAngular(self):
        rc, idx = self._require_owner()
        rc._ctrl.reset_integrators(idx, 2)

    def getUnitMassForce(self):
        """MotionForceTask.h:266, of the last tick (introspection on)"""
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_task_forces(idx)[0]

    def getCurrentLinearVelocity(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_velocity(idx)[0]

    def getCurrentAngularVelocity(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_velocity(idx)[1]

    def sigmaForce(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_sigma(idx)[0]

    def sigmaPosition(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_sigma(idx)[1]

    def sigmaMoment(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_sigma(idx)[2]

    def sigmaOrientation(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_sigma(idx)[3]

    def setPosControlGainsUnsafe(self, kp, kv, ki):
        """MotionForceTask.h:283 (MotionForceTask.cpp: no sign check, per-axis values)"""
        for n, v in zip(("kp_pos", "kv_pos", "ki_pos"), (kp, kv, ki)):
            v = np.broadcast_to(np.asarray(v, dtype=float), (3,))
            for i in range(3):
                getattr(self._cfg, n)[i] = v[i]
        self._sync_cfg()

    def setOriControlGainsUnsafe(self, kp, kv, ki):
        for n, v in zip(("kp_ori", "kv_ori", "ki_ori"), (kp, kv, ki)):
            v = np.broadcast_to(np.asarray(v, dtype=float), (3,))
            for i in range(3):
                getattr(self._cfg, n)[i] = v[i]
        self._sync_cfg()

    def getForceControlGains(self):
        return [(self._cfg.kp_force[0], self._cfg.kv_force[0], self._cfg.ki_force[0])]

    def getMomentControlGains(self):
        return [(self._cfg.kp_moment[0], self._cfg.kv_moment[0], self._cfg.ki_moment[0])]

    def handleAllSingularitiesAsType1(self, flag=True):
        """MotionForceTask.h:697"""
        self._cfg.enforce_type_1_strategy = int(bool(flag))
        self._sync_cfg()

    def setType1Posture(self, q_des):
        """MotionForceTask.h:706; q_des [n][B]"""
        rc, idx = self._require_owner()
        rc._ctrl.set_mft_type1_posture(idx, q_des)

    def getForceMotionSingleAxis(self):
        return np.array(self._cfg.force_axis[:])

    def getMomentRotMotionSingleAxis(self):
        return np.array(self._cfg.moment_axis[:])

    def getSigmaValues(self):
        rc, idx = self._require_owner()
        return rc._ctrl.get_mft_singularity(idx)[0]

    def _flush(self):
        if self._owner and self._pending:
            rc, idx = self._owner
            p = self._pending
            if any(k in p for k in ("pos", "rot", "v", "w", "a", "alpha")):
                rc._ctrl.set_mft_goals(idx, p.get("pos"), p.get("rot"), p.get("v"), p.get("w"), p.get("a"), p.get("alpha"))
            if "f" in p or "m" in p:
                rc._ctrl.set_mft_goal_wrench(idx, p.get("f"), p.get("m"))
            if "sf" in p or "sm" in p:
                rc._ctrl.set_mft_sensed_wrench(idx, p.get("sf"), p.get("sm"))
            self._pending = {}


class RobotController:
    """reference src/RobotController.h:25-40: same ctor checks, same entry points, batched."""

    def __init__(self, robot, tasks, introspection=False):
        if len(tasks) == 0:
            raise ValueError("RobotController must have at least one task")
        for t in tasks:
            if t.getConstRobotModel() is not robot:
                raise ValueError("All tasks must have the same robot model in RobotController")
        self._robot = robot
        self._tasks = list(tasks)
        self._ctrl = Controller(robot.model, [t._cfg for t in tasks], robot.batch, robot.device, introspection)
        robot._apply_payloads(self._ctrl)
        robot._controller = self
        self._ctrl.set_state(robot.q(), robot.dq())
        self._ctrl.reinitialize()  # tasks are constructed at the model's current state
        for i, t in enumerate(self._tasks):
            t._owner = (self, i)
            t._flush()

    def updateControllerTaskModels(self):
        self._ctrl.update_task_models()

    def computeControlTorques(self, out=None):
        return self._ctrl.compute_control_torques(True, out)

    def tick(self, out=None):
        """fused updateControllerTaskModels() + computeControlTorques(): one kernel launch"""
        return self._ctrl.tick(out)

    def enableGravityCompensation(self, enable=True):
        self._ctrl.enable_gravity_compensation(enable)

    def reinitializeTasks(self, mask=None):
        """mask [B] (bool / uint8): only for the robots it selects"""
        if mask is None:
            self._ctrl.reinitialize()
        else:
            self._ctrl.reinitialize_robots(mask)

    def resetRobots(self, mask, q=None, dq=None):
        """Controller.reset_robots; the model's host copy of the state follows for the selected robots (host arrays only:
        with device tensors the state lives on the device, as under BatchedSimulation)"""
        self._ctrl.reset_robots(mask, q, dq)
        if not hasattr(mask, "data_ptr"):
            sel = np.asarray(mask).astype(bool)
            for name, new in (("_q", q), ("_dq", dq)):
                cur = getattr(self._robot, name)
                if new is not None and isinstance(cur, np.ndarray):
                    cur = np.array(cur, dtype=np.float64)
                    cur[:, sel] = np.asarray(new, dtype=np.float64)[:, sel]
                    setattr(self._robot, name, cur)

    def createSnapshotBank(self, capacity, what=_abi.SNAP_EPISODE):
        """Controller.snapshot_bank: whole robot states saved to and restored from device memory"""
        return self._ctrl.snapshot_bank(capacity, what)

    def getTaskNames(self):
        return [t.getTaskName() for t in self._tasks]

    def _by_name(self, name, kind, label):
        for t in self._tasks:
            if t.getTaskName() == name:
                if t.getTaskType() != kind:
                    raise ValueError(f"Task {name} is not a {label}, and cannot be casted as such in RobotController::GetTaskByName")
                return t
        raise ValueError(f"Task {name} not found in RobotController::GetTaskByName")

    def getJointTaskByName(self, name):
        return self._by_name(name, _abi.JOINT_TASK, "JointTask")

    def getMotionForceTaskByName(self, name):
        return self._by_name(name, MOTION_FORCE_TASK, "MotionForceTask")


class BatchedSimulation:
    """Stands in for Sai2Simulation in the examples' loops (examples/05-...cpp:215-236): rigid-body dynamics
    of the batch, state resident on the device. Without setJointTorques, integrate() consumes the torques
    of the controller's last computeControlTorques() / tick() without a host round trip."""

    def __init__(self, controller, timestep=0.001, substeps=1):
        if timestep <= 0 or substeps < 1:
            raise ValueError("simulation timestep must be positive")
        self._c, self._dt, self._substeps, self._gravity, self._tau = controller, float(timestep), int(substeps), False, None

    def setTimestep(self, dt):
        if dt <= 0:
            raise ValueError("simulation timestep must be positive")
        self._dt = float(dt)

    def enableGravity(self, on=True):
        self._gravity = bool(on)

    def setJointTorques(self, tau):
        self._tau = tau

    def integrate(self):
        self._c._ctrl.sim_step(self._tau, self._dt, self._substeps, self._gravity)
        self._tau = None

    def getJointPositions(self):
        return self._c._ctrl.get_state()[0]

    def getJointVelocities(self):
        return self._c._ctrl.get_state()[1]

    def createSnapshotBank(self, capacity, what=_abi.SNAP_EPISODE | _abi.SNAP_ENVIRONMENT):
        """Controller.snapshot_bank; by default with the plant's per-robot environment (payloads, planes, joint rows, pushes)"""
        return self._c._ctrl.snapshot_bank(capacity, what)

    # -- joint dynamics of the plant (Controller.set_joint_dynamics)
    def setJointDynamics(self, *args, **kwargs):
        self._c._ctrl.set_joint_dynamics(*args, **kwargs)

    def clearJointDynamics(self):
        self._c._ctrl.clear_joint_dynamics()

    def getJointDynamicsState(self):
        return self._c._ctrl.get_joint_dynamics_state()

    # -- external wrench on a link of the plant (Controller.set_external_wrench)
    def setExternalWrench(self, *args, **kwargs):
        self._c._ctrl.set_external_wrench(*args, **kwargs)

    def clearExternalWrench(self):
        self._c._ctrl.clear_external_wrench()

    def getExternalWrenchState(self):
        return self._c._ctrl.get_external_wrench_state()

    def robotsPushed(self):
        return self._c._ctrl.robots_pushed()

    # -- actuator and force-sensor models (Controller.set_hardware)
    def setHardware(self, *args, **kwargs):
        self._c._ctrl.set_hardware(*args, **kwargs)

    def clearHardware(self):
        self._c._ctrl.clear_hardware()

    def getHardwareState(self):
        return self._c._ctrl.get_hardware_state()

    # -- joint sensors (Controller.set_joint_sensor)
    def setJointSensor(self, *args, **kwargs):
        self._c._ctrl.set_joint_sensor(*args, **kwargs)

    def clearJointSensor(self):
        self._c._ctrl.clear_joint_sensor()

    def jointSensorState(self):
        return self._c._ctrl.joint_sensor_state()

    def measuredState(self):
        return self._c._ctrl.get_measured_state()

    # -- contact of the plant (Controller.set_contact); the force sensor writes the sensed rows of one MotionForceTask
    def setContactPlanes(self, *args, **kwargs):
        self._c._ctrl.set_contact(*args, **kwargs)

    def clearContact(self):
        self._c._ctrl.clear_contact()

    def _sensor(self, task):
        cfg, rows = self._c._ctrl.get_contact()
        if cfg.n_points == 0:
            raise ValueError("no contact is set (setContactPlanes)")
        cfg.sensor_task = int(task)
        self._c._ctrl.set_contact(cfg, None, rows[0:3], rows[3:6], rows[6], rows[7], rows[8])

    def attachForceSensor(self, task):
        """the MotionForceTask (index in the controller's hierarchy) whose sensed rows the simulated sensor writes"""
        self._sensor(task)

    def detachForceSensor(self):
        self._sensor(-1)

    def getContactState(self):
        return self._c._ctrl.get_contact_state()

    def robotsInContact(self):
        return self._c._ctrl.robots_in_contact()

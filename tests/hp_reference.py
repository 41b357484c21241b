"""One control tick of a task hierarchy in mpmath at 40 significant digits (test infrastructure): the ground truth the
singular branch of every kernel route, and the CPU oracle, are held to (tests/test_hp_reference.py,
tests/test_gpu_hp_singular.py through the fixture tests/golden/hp_singular.npz).

mpmath and numpy only, nothing of the product's or the oracle's code. The robot is read from its URDF text the way
tests/urdf_np.py reads it (joint origin, then a rotation about / translation along the joint's <axis>; fixed joints'
bodies move with the link they hang on), every float64 of the file taken as the exact number it is, every sine and
cosine evaluated at the working precision. The tasks are plain dicts of the numbers a task config carries (gains,
thresholds, the perturbation step, the partial projection): tests/golden/make_hp_golden.py reads them from the
product's own defaults.

The SingularityHandler (SingularityHandler.cpp:75-368, read as tests/golden/make_golden.py reads it): thin SVD of
J N_prec with every right singular vector oriented "largest-magnitude component positive", the split at the first
ratio s_i / s_0 below s_max, alpha = clip((rho - s_min) / (s_max - s_min)), s_abs_tol; Lambda_ns, Lambda_s and
Lambda_joint for full dynamic decoupling, BIE and impedance; the type-1 / type-2 classification by FK perturbation with
the singular-vector-sign setting; the history ring and its counters, q_prior, the type-2 joint-limit directions; the
effort clamp of tau_s and tau = tau_ns + alpha tau_s + (1 - alpha) tau_joint.

The rigid-body dynamics of the simulation harness (csrc/sai2b_sim.hip), derived without a Newton-Euler recursion:
bias() sums b = C(q, dq) dq + g(q) over the bodies from their velocity-product accelerations, found by differentiating
the body poses along q + t dq; bias_lagrange() is the Lagrangian form from derivatives of M; sim_step() restates the
integrator (the torque held over the period, `substeps` semi-implicit Euler steps).

The task laws in full (MotionForceTask.cpp:278-509 with sigmaForce / Position / Moment / Orientation, getGoalForce /
Moment and updateSensedForceAndMoment :805-828, JointTask.cpp:294-350, the handler's two arguments
SingularityHandler.cpp:297-368), read from that text: force and moment spaces of dimension 0-3 in the world or the
compliant frame, the goal wrench, the sensed wrench through the sensor frame with its lever arm, open- and closed-loop
force and moment with their integrators and the feedback limit on the norm, the feed-forward whose two gains hang on the
closed-loop *force* flag, the motion integrators, velocity saturation through the pseudo-inverse of k_v, per-axis gains;
the JointTask's integrator and per-joint saturation. The passivity observer, the trajectory generators and contact are
not restated. The held fixtures of these laws are tests/golden/hp_force.npz (tests/test_hp_force_reference.py).
A force or moment axis is normalised at the working precision, as the reference normalises what it is given.

The simulated plant beyond the rigid body (contact, joint dynamics, the external wrench, the plant payload, the sensor
and status rows): plant_step() and plant_report() at the end of this file, written from DESIGN's laws with the point
Jacobians formed explicitly and the implicit system solved by LU; the fixture is tests/golden/hp_plant.npz
(tests/test_hp_plant.py), and the planted errors of that test are listed there.

HOOKS plants errors for tests/test_hp_reference.py, tests/test_hp_force_reference.py and tests/test_hp_dynamics.py (each
must be caught by the checker): alpha_rel, flip_vs_type2, no_clamp, pinv_ls, kv1_for_kv2, stale_q_prior;
ff_through_lambda, kff_moment_own_flag, sensor_no_lever, integ_after_use, sat_componentwise, vsat_no_pinv,
type2_from_fu_only, goal_wrench_not_rotated; pris_coriolis_half, no_gyroscopic, explicit_euler."""
import copy
import re
import xml.etree.ElementTree as ET

import mpmath
import numpy as np
from mpmath import mp, mpf

mp.dps = 40
EPS = 2.0 ** -52
HOOKS = {}
FULL, BIE, IMPEDANCE = 0, 1, 2


def _nums(text, n, default):
    if text is None:
        return [float(x) for x in default]
    out = [float(re.match(r"[-+]?(\d+\.?\d*([eE][-+]?\d+)?|\.\d+([eE][-+]?\d+)?)", tok).group(0)) for tok in text.split()]
    assert len(out) == n, text
    return out


def M_(a):
    """float / nested list / numpy array -> object array of exact mpf"""
    a = np.asarray(a)
    if a.dtype != object:
        a = a.astype(float)
    return np.vectorize(lambda v: mpf(v) if not isinstance(v, mpf) else v, otypes=[object])(a)


def zeros(*shape):
    return np.full(shape, mpf(0), dtype=object)


def eye(n):
    out = zeros(n, n)
    for i in range(n):
        out[i, i] = mpf(1)
    return out


def inv(a):
    return np.array(mp.inverse(mp.matrix(a.tolist())).tolist(), dtype=object)


def svd(a):
    """thin SVD a = U diag(s) V^T, s descending"""
    U, S, Vt = mp.svd_r(mp.matrix(a.tolist()), full_matrices=False)
    return np.array(U.tolist(), dtype=object), np.array([S[i] for i in range(S.rows)], dtype=object), np.array(Vt.tolist(), dtype=object).T


def sym_pinv(a):
    """pseudo-inverse of a symmetric matrix, singular values below n eps s_0 dropped (the oracle's cut-off)"""
    U, s, V = svd(a)
    n = a.shape[0]
    d = [1 / x if x > n * EPS * s[0] and x > 0 else mpf(0) for x in s]
    return V @ np.diag(np.array(d, dtype=object)) @ U.T


def norm_inf(v):
    return max(abs(x) for x in np.ravel(v))


def norm_fro(a):
    return mp.sqrt(sum(x * x for x in np.ravel(a)))


def _rpy(r):
    cr, sr, cp, sp, cy, sy = mp.cos(r[0]), mp.sin(r[0]), mp.cos(r[1]), mp.sin(r[1]), mp.cos(r[2]), mp.sin(r[2])
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]], dtype=object)


def _skew(a):
    z = mpf(0)
    return np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], dtype=object)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=object)


class Model:
    """a serial chain from URDF text; every number of the file as a float64, made exact mpf where it is used"""

    def __init__(self, text, base=None):
        """base: (position, rotation) of the root link in the world (Sai2Model::setTRobotBase), float64 numbers; the
        rotation is taken as the orthogonal matrix nearest to it (U V^T of its SVD, at the working precision): a rigid
        motion, as the product's own (it keeps the base as roll-pitch-yaw angles)"""
        if base is not None:
            U, _, V = svd(M_(base[1]))
            base = (M_(base[0]), U @ V.T)
        self.base = base
        root = ET.fromstring(text)
        self.links = {}
        for l in root.findall("link"):
            inn = l.find("inertial")
            if inn is None:
                self.links[l.get("name")] = None
                continue
            o, I = inn.find("origin"), inn.find("inertia")
            g = lambda k: float(I.get(k, "0")) if I is not None else 0.0
            self.links[l.get("name")] = dict(
                m=float(inn.find("mass").get("value")), com=_nums(o.get("xyz") if o is not None else None, 3, [0, 0, 0]),
                rpy=_nums(o.get("rpy") if o is not None else None, 3, [0, 0, 0]),
                I=[[g("ixx"), g("ixy"), g("ixz")], [g("ixy"), g("iyy"), g("iyz")], [g("ixz"), g("iyz"), g("izz")]])
        self.joints, children = [], set()
        for j in root.findall("joint"):
            o, ax, lim = j.find("origin"), j.find("axis"), j.find("limit")
            self.joints.append(dict(type=j.get("type"), parent=j.find("parent").get("link"), child=j.find("child").get("link"),
                                    xyz=_nums(o.get("xyz") if o is not None else None, 3, [0, 0, 0]),
                                    rpy=_nums(o.get("rpy") if o is not None else None, 3, [0, 0, 0]),
                                    axis=_nums(ax.get("xyz") if ax is not None else None, 3, [1, 0, 0]),
                                    lower=float(lim.get("lower", "0")) if lim is not None else 0.0,
                                    upper=float(lim.get("upper", "0")) if lim is not None else 0.0,
                                    effort=float(lim.get("effort", "0")) if lim is not None else 0.0))
            children.add(self.joints[-1]["child"])
        (self.root,) = [n for n in self.links if n not in children]
        self.order, cur = [], [self.root]  # joints parent before child
        while cur:
            nxt = []
            for j in self.joints:
                if j["parent"] in cur:
                    self.order.append(j)
                    nxt.append(j["child"])
            cur = nxt
        self.moving = [j for j in self.order if j["type"] != "fixed"]
        self.dof = len(self.moving)
        self.lower = np.array([j["lower"] for j in self.moving])
        self.upper = np.array([j["upper"] for j in self.moving])
        self.effort = np.array([j["effort"] for j in self.moving])

    def poses(self, q):
        """{link: (R, p, index of the last moving joint at or before it, -1 for none)}, per moving joint (axis, origin, type)"""
        out = {self.root: (eye(3), zeros(3), -1) if self.base is None else (self.base[1], self.base[0], -1)}
        jinfo = [None] * self.dof
        for j in self.order:
            Rp, pp, mv = out[j["parent"]]
            R, p = Rp @ _rpy([mpf(x) for x in j["rpy"]]), pp + Rp @ M_(j["xyz"])
            if j["type"] != "fixed":
                k = self.moving.index(j)
                a = M_(j["axis"])
                a = a / mp.sqrt(a @ a)
                aw = R @ a
                if j["type"] == "prismatic":
                    p = p + aw * q[k]
                else:
                    K = _skew(a)
                    R = R @ (eye(3) + mp.sin(q[k]) * K + (1 - mp.cos(q[k])) * (K @ K))
                jinfo[k] = (aw, p, j["type"])
                mv = k
            out[j["child"]] = (R, p, mv)
        return out, jinfo

    def jacobian(self, pos, jinfo, link, point):
        R, p, mv = pos[link]
        x = p + R @ point
        J = zeros(6, self.dof)
        for k in range(mv + 1):
            aw, o, typ = jinfo[k]
            if typ == "prismatic":
                J[:3, k] = aw
            else:
                J[:3, k] = _cross(aw, x - o)
                J[3:, k] = aw
        return J, x, R

    def dynamics(self, q, gravity=(0, 0, -9.81)):
        """pose tables, mass matrix M = sum_k m_k Jv^T Jv + Jw^T I_k Jw, gravity vector"""
        pos, jinfo = self.poses(q)
        n = self.dof
        M, g = zeros(n, n), zeros(n)
        gr = M_(gravity)
        for name, body in self.links.items():
            if body is None or pos[name][2] < 0:
                continue
            J, _, R = self.jacobian(pos, jinfo, name, M_(body["com"]))
            Ro = R @ _rpy([mpf(x) for x in body["rpy"]])
            Iw = Ro @ M_(body["I"]) @ Ro.T
            m = mpf(body["m"])
            M += m * (J[:3].T @ J[:3]) + J[3:].T @ Iw @ J[3:]
            g -= m * (J[:3].T @ gr)
        return pos, jinfo, M, g

    def frame(self, pos, jinfo, task):
        J, x, R = self.jacobian(pos, jinfo, task["link"], M_(task["point"]))
        return J, x, R @ M_(task["frot"])


def orientation_error(Rd, Rc):
    e = zeros(3)
    for i in range(3):
        e = e - _cross(Rc[:, i], Rd[:, i]) / 2
    return e


def opspace(J, Minv):
    L = inv(J @ Minv @ J.T)
    Jbar = Minv @ J.T @ L
    return L, Jbar, eye(Minv.shape[0]) - Jbar @ J


def bie_minv(M, thr):
    MB = M.copy()
    for i in range(M.shape[0]):
        if MB[i, i] < thr:
            MB[i, i] = mpf(thr)
    return inv(MB)


def new_state(model, tasks):
    """per MotionForceTask: the SingularityHandler's state after construction and the twelve integrators (position,
    orientation, force, moment); per JointTask: its integrator"""
    return [dict(types=[], hist=[], c1=0, c2=0, q_prior=(M_(model.lower) + M_(model.upper)) / 2, t2dir=[1] * model.dof,
                 integ=zeros(12))
            if t["kind"] == "mft" else dict(integ=zeros(np.asarray(t["S"]).shape[0])) for t in tasks]


def _mft_update(model, t, st, q, M, Minv, MiB, Jw, N_prec, pose0, pert, types_override, out):
    n = model.dof
    J = M_(t["P"]) @ Jw
    Jp = J @ N_prec
    out["Jp"] = Jp
    if pert is not None:
        Jp = Jp + pert["Jp"]
    U, s, V = svd(Jp)
    for j in range(V.shape[1]):
        k = max(range(n), key=lambda i: abs(V[i, j]))
        if V[k, j] < 0:
            V[:, j], U[:, j] = -V[:, j], -U[:, j]
    rank = min(t["rank"], len(s))
    smin, smax = mpf(t["s_min"]), mpf(t["s_max"])
    if s[0] < t["s_abs_tol"]:
        alpha, split = mpf(0), 0
    else:
        alpha, split = mpf(1), rank
        for i in range(1, rank):
            rho = s[i] / s[0]
            if rho < smax:
                a = (rho - smin) / (smax - smin)
                if "alpha_rel" in HOOKS:
                    a = a * (1 + mpf(HOOKS["alpha_rel"]))
                alpha, split = min(max(a, mpf(0)), mpf(1)), i
                break
    ns, sc = split, rank - split
    m = dict(J=J, Jp=Jp, alpha=alpha, ns=ns, sc=sc, have_post=False, sv=s)
    if ns:
        m["U_ns"] = U[:, :ns]
        m["J_ns"] = m["U_ns"].T @ Jp
        m["L_ns"], _, m["N_ns"] = opspace(m["J_ns"], Minv)
    if sc:
        m["U_s"], m["V_s"] = U[:, split:rank], V[:, split:rank]
        m["J_s"] = m["U_s"].T @ Jp
        A = m["J_s"] @ Minv @ m["J_s"].T
        m["L_s"] = sym_pinv(A) if ns == 0 or "pinv_ls" in HOOKS else inv(A)
    if ns == 0:
        Nt = N_prec
    elif sc == 0 or not t["enforce_handling"]:
        Nt = m["N_ns"]
    else:
        m["J_post"] = m["V_s"].T @ m["N_ns"] @ N_prec
        m["L_joint"], _, Np = opspace(m["J_post"], Minv)
        Nt = Np @ m["N_ns"]
        m["have_post"] = True
    dec = t["decoupling"]
    for key, Jk, on in (("ns", "J_ns", ns), ("s", "J_s", sc), ("joint", "J_post", m["have_post"])):
        if not on:
            continue
        if dec == IMPEDANCE:
            m["Lm_" + key] = eye(m[Jk].shape[0])
        elif dec == BIE:
            m["Lm_" + key] = inv(m[Jk] @ MiB @ m[Jk].T)
        else:
            m["Lm_" + key] = m["L_" + key]
    m["N_total"] = Nt @ N_prec
    # classification (SingularityHandler.cpp:230-295)
    if (len(st["types"]) == 0 or st["c2"] > st["c1"]) and "stale_q_prior" not in HOOKS:
        st["q_prior"] = q.copy()
    out["d1"] = []
    if sc == 0:
        st.update(types=[], hist=[], c1=0, c2=0)
    else:
        x0, R0 = pose0
        types = []
        for i in range(sc):
            if types_override is not None:
                types.append(types_override[i])
                continue
            moved, dmin = [], []
            for step in (t["perturb"], -t["perturb"]):
                qp = q + mpf(step) * m["V_s"][:, i]
                pos, jinfo = model.poses(qp)
                _, x1, R1 = model.frame(pos, jinfo, t)
                d = np.concatenate([x1 - x0, orientation_error(R1, R0)])
                dm = abs(d @ m["U_s"][:, i])
                moved.append(dm > t["type1_tol"])
                dmin.append(dm)
            out["d1"] += dmin
            sgn = t["sv_sign"]
            t1 = {0: moved[0], 1: moved[1], 2: moved[0] or moved[1], 3: moved[0] and moved[1]}[sgn]
            types.append(1 if t1 else 2)
        st["types"] = types
        st["hist"].append(1 if 1 in types else 2)
        st["c1" if 1 in types else "c2"] += 1
        if len(st["hist"]) > t["buffer"]:
            st["c1" if st["hist"].pop(0) == 1 else "c2"] -= 1
    out.update(s0=s[0], ratios=[x / s[0] for x in s], alpha=alpha, sc=sc, types=list(st["types"]), c1=st["c1"], c2=st["c2"])
    return m


def _sigma(dim, axis, Rp, Pb):
    """sigmaForce / sigmaMoment (MotionForceTask.cpp:892-966): the selection of a space of dimension `dim` about `axis`
    (normalised as parametrizeForceMotionSpaces does, :848), Rp the rotation of the parametrisation, Pb the 3 x 3 block
    of the partial projection"""
    if dim == 0:
        return zeros(3, 3)
    if dim == 3:
        return Pb
    a = M_(axis)
    a = Rp @ (a / mp.sqrt(a @ a))
    aa = np.outer(a, a)
    return Pb @ (aa if dim == 1 else eye(3) - aa) @ Pb.T


def _saturate(vec, lim, key, out):
    """vec scaled down to the norm lim when its norm exceeds it; the decision recorded"""
    nv = mp.sqrt(vec @ vec)
    out.setdefault("norms", []).append((nv, lim))
    out[key] = bool(nv > lim)
    if "sat_componentwise" in HOOKS:
        return np.array([min(max(c, -mpf(lim)), mpf(lim)) for c in vec], dtype=object)
    return vec * (mpf(lim) / nv) if nv > lim else vec


def _gain_pinv(kv):
    """Sai2Model::computePseudoInverse of a diagonal gain matrix: a zero gain gives 0"""
    if "vsat_no_pinv" in HOOKS:
        return np.array([1 / c if c != 0 else mpf(1) for c in kv], dtype=object)
    return np.array([1 / c if c != 0 else mpf(0) for c in kv], dtype=object)


def _mft_law(t, st, J, dq, x, R, goal, out):
    """MotionForceTask::computeTorques up to the singularity handler (MotionForceTask.cpp:306-506), the passivity
    observer off and the desired motion the goal: (F_u, F_f), the integrators of st advanced"""
    P = M_(t["P"])
    Pp, Po = P[:3, :3], P[3:, 3:]
    Rp = R if t.get("in_frame") else eye(3)
    sf = _sigma(t.get("fdim", 0), t.get("faxis"), Rp, Pp)
    sm = _sigma(t.get("mdim", 0), t.get("maxis"), Rp, Po)
    sp, so = Pp @ (eye(3) - sf) @ Pp.T, Po @ (eye(3) - sm) @ Po.T
    v, w = J[:3] @ dq, J[3:] @ dq
    dt = mpf(t.get("dt", 0))
    late = "integ_after_use" in HOOKS
    old = st["integ"].copy()
    new = old.copy()
    g3 = lambda key: M_(t[key]) if key in t else zeros(3)
    # goal and sensed wrench (:755-769, :805-828)
    gf = Rp @ M_(goal["f"]) if "f" in goal else zeros(3)
    gm = Rp @ M_(goal["m"]) if "m" in goal else zeros(3)
    if "goal_wrench_not_rotated" in HOOKS and "f" in goal:
        gf, gm = M_(goal["f"]), M_(goal["m"])
    fs, ms = zeros(3), zeros(3)
    if "sf" in goal:
        Rs, ps = M_(np.asarray(t["sensor_rot"]).reshape(3, 3)), M_(t["sensor_pos"])
        fc = Rs @ M_(goal["sf"])
        mc = Rs @ M_(goal["sm"]) + (zeros(3) if "sensor_no_lever" in HOOKS else _cross(ps, fc))
        fs, ms = R @ fc, R @ mc
    out.update(sat_f=False, sat_m=False, sat_v=False, sat_w=False)
    cl_f, cl_m = bool(t.get("cl_force")), bool(t.get("cl_moment"))
    # force (:327-354; POPCExplicitForceControl.cpp:33-35 with the observer off) and moment (:357-383)
    if cl_f:
        new[6:9] = old[6:9] + sf @ (fs - gf) * dt
        fb = sf @ (-g3("kp_f") * (fs - gf) - g3("ki_f") * (old if late else new)[6:9])
        fb = _saturate(fb, t["max_f"], "sat_f", out)
        f_force = sf @ fb - g3("kv_f") * (sf @ v)
    else:
        f_force = sf @ (-g3("kv_f") * v)
    if cl_m:
        new[9:12] = old[9:12] + sm @ (ms - gm) * dt
        fb = sm @ (-g3("kp_m") * (ms - gm) - g3("ki_m") * (old if late else new)[9:12])
        fb = _saturate(fb, t["max_m"], "sat_m", out)
        f_moment = sm @ (fb - g3("kv_m") * w)
    else:
        f_moment = sm @ (-g3("kv_m") * w)
    # linear motion (:409-437)
    gpos, grot = M_(goal["pos"]), M_(np.asarray(goal["rot"]).reshape(3, 3))
    kp, kv, ki = M_(t["kp_pos"]), M_(t["kv_pos"]), g3("ki_pos")
    new[0:3] = old[0:3] + sp @ (x - gpos) * dt
    ip = (old if late else new)[0:3]
    if t.get("vsat"):
        kvi = _gain_pinv(kv)
        des = _saturate(-kp * kvi * (sp @ (x - gpos)) - ki * kvi * ip, t["lin_vsat"], "sat_v", out)
        f_pos = sp @ (M_(goal["a"]) - kv * (v - des))
    else:
        f_pos = sp @ (M_(goal["a"]) - kp * (x - gpos) - kv * (v - M_(goal["v"])) - ki * ip)
    # angular motion (:439-468)
    kp, kv, ki = M_(t["kp_ori"]), M_(t["kv_ori"]), g3("ki_ori")
    step = so @ orientation_error(grot, R)
    new[3:6] = old[3:6] + step * dt
    io = (old if late else new)[3:6]
    if t.get("vsat"):
        kvi = _gain_pinv(kv)
        des = _saturate(-kp * kvi * step - ki * kvi * io, t["ang_vsat"], "sat_w", out)
        f_ori = so @ (M_(goal["alpha"]) - kv * (w - des))
    else:
        f_ori = so @ (M_(goal["alpha"]) - kp * step - kv * (w - M_(goal["w"])) - ki * io)
    # feed-forward (:480-487): both halves scaled under the closed-loop *force* flag
    ff_f, ff_m = sf @ gf, sm @ gm
    if cl_f:
        ff_f = ff_f * mpf(t["kff_f"])
    if cl_m if "kff_moment_own_flag" in HOOKS else cl_f:
        ff_m = ff_m * mpf(t["kff_m"])
    st["integ"] = new
    out["integ"] = new.copy()
    return np.concatenate([f_pos, f_ori]), np.concatenate([f_force + ff_f, f_moment + ff_m])


def _mft_torques(model, t, st, m, q, dq, x, R, goal, out):
    """SingularityHandler::computeTorques(unit_mass_force, force_related_terms) (SingularityHandler.cpp:297-368)"""
    n = model.dof
    out["integ"] = st["integ"].copy()
    if t["rank"] == 0:
        return zeros(n)
    Fu, Ff = _mft_law(t, st, m["J"], dq, x, R, goal, out)
    ns, sc = m["ns"], m["sc"]
    out["Ff_norm"] = float(mp.sqrt(Ff @ Ff))

    def through(key, L):
        Ut = m["U_" + key].T
        if "ff_through_lambda" in HOOKS:
            return m["J_" + key].T @ (L @ (Ut @ Fu + Ut @ Ff))
        return m["J_" + key].T @ (L @ (Ut @ Fu) + Ut @ Ff)

    if len(st["types"]) == 0:
        return through("ns", m["Lm_ns"]) if ns else zeros(n)
    if t["decoupling"] == IMPEDANCE:
        return through("ns", eye(ns)) if ns else zeros(n)
    if ns == 0:
        return zeros(n)
    tau_ns = through("ns", m["Lm_ns"])
    if not t["enforce_handling"]:
        return tau_ns
    V_s, J_post, Lj = m["V_s"], m["J_post"], m["Lm_joint"]
    if st["c1"] > st["c2"] or t["enforce_type_1"]:
        ut = -mpf(t["kp1"]) * (q - st["q_prior"]) - mpf(t["kv1"]) * dq
        tau_j = J_post.T @ (Lj @ (V_s.T @ ut))
        out["branch"] = 1
    else:
        lo, hi = model.lower, model.upper
        for i in range(n):
            if V_s[i, 0] != 0:
                if abs(q[i] - mpf(hi[i])) < t["t2_angle"]:
                    st["t2dir"][i] = -1
                elif abs(q[i] - mpf(lo[i])) < t["t2_angle"]:
                    st["t2dir"][i] = 1
        F = Fu if "type2_from_fu_only" in HOOKS else Fu + Ff
        nF = mp.sqrt(F @ F)
        fTd = (F / nF if nF > 0 else F) @ m["U_s"][:, 0]
        ut = np.array([st["t2dir"][i] * abs(fTd) * mpf(t["t2_ratio"]) * mpf(model.effort[i]) for i in range(n)], dtype=object)
        Vt = -V_s if "flip_vs_type2" in HOOKS else V_s
        kv2 = t["kv1"] if "kv1_for_kv2" in HOOKS else t["kv2"]
        tau_j = J_post.T @ (Vt.T @ ut) + J_post.T @ (Lj @ (V_s.T @ (-mpf(kv2) * dq)))
        out["branch"] = 2
    tau_s = through("s", m["Lm_s"])
    eff = M_(model.effort)
    out["clamped"] = int(sum(abs(tau_s[i]) > eff[i] for i in range(n)))
    if "no_clamp" not in HOOKS:
        tau_s = np.array([min(max(tau_s[i], -eff[i]), eff[i]) for i in range(n)], dtype=object)
    a = m["alpha"]
    return tau_ns + a * tau_s + (1 - a) * tau_j


def _jt_update(t, M, Minv, MiB, N_prec, out):
    n = M.shape[0]
    S = M_(t["S"])
    Jp = S @ N_prec
    U, s, _ = svd(Jp)
    out["range_ratio"] = [x / s[0] for x in s[1:]]
    k = len(s)
    for i in range(len(s) - 1, 0, -1):  # the range basis of sai2-model, tolerance 1e-3 on s_i / s_0
        if s[i] / s[0] < 1e-3:
            k -= 1
        else:
            break
    if s[0] < 1e-3:
        return dict(k=0, N_total=eye(n) @ N_prec, Jp=Jp)
    Rb = eye(S.shape[0]) if k == S.shape[0] else U[:, :k]
    Jr = Rb.T @ Jp
    Mp, _, N = opspace(Jr, Minv)
    dec = t["decoupling"]
    Mpm = Mp if dec == FULL else (inv(Jr @ MiB @ Jr.T) if dec == BIE else eye(k))
    return dict(k=k, Rb=Rb, Jp=Jp, Mp=Mp, Mpm=Mpm, S=S, N_total=N @ N_prec)


def _jt_torques(t, st, m, q, dq, Minv, tau_prec, goal, out):
    """JointTask::computeTorques (JointTask.cpp:294-356) with the compensation of :285-292"""
    n = len(q)
    out["integ"] = st["integ"].copy()
    if m["k"] == 0:  # (:302-306: nothing advances)
        return zeros(n)
    S, Rb, Jp = m["S"], m["Rb"], m["Jp"]
    kp, kv, ki = M_(t["kp"]), M_(t["kv"]), M_(t["ki"]) if "ki" in t else zeros(S.shape[0])
    e = S @ q - M_(goal["q"])
    old = st["integ"]
    st["integ"] = old + e * mpf(t.get("dt", 0))
    out["integ"] = st["integ"].copy()
    integ = old if "integ_after_use" in HOOKS else st["integ"]
    out["sat_jt"] = False
    if t.get("vsat"):
        des = -kp * _gain_pinv(kv) * e - ki * _gain_pinv(kv) * integ
        sat = M_(t["sat"])
        out["jt_des"] = [(abs(des[i]), sat[i]) for i in range(len(des))]
        out["sat_jt"] = bool(any(abs(des[i]) > sat[i] for i in range(len(des))))
        des = np.array([min(max(des[i], -sat[i]), sat[i]) for i in range(len(des))], dtype=object)
        f = -kv * (S @ dq - des)
    else:
        f = -kp * e - kv * (S @ dq - M_(goal["dq"])) - ki * integ
    xx = m["Mp"] @ (Rb.T @ M_(goal["ddq"])) + m["Mpm"] @ (Rb.T @ f)
    tau = Jp.T @ (Rb @ xx)
    return tau - Jp.T @ (Rb @ (m["Mp"] @ (Rb.T @ (S @ (Minv @ tau_prec)))))


def tick(model, tasks, state, q, dq, goals, pert=None, types_override=None, kin=None, gravity_comp=False):
    """one tick of the hierarchy: update_task_models() then compute_control_torques() with the compensation terms,
    g(q) added when gravity_comp (RobotController.cpp:70-72).
    state (new_state) is advanced. pert: additive perturbations of the model quantities {M, Jp[t], x[t], R[t], dq}, and
    where present of the sensed wrench {sf[t], sm[t]} and of the carried integrators {integ[t]} (added to state first).
    types_override[t]: the types of the classification (the perturbed re-evaluations keep the unperturbed decisions).
    kin: the FK quantities of an earlier call at the same q. Returns (tau, info per task, kin)."""
    q, dq = M_(q), M_(dq)
    if kin is None:
        pos, jinfo, M, g = model.dynamics(q)
        frames = [model.frame(pos, jinfo, t) if t["kind"] == "mft" else None for t in tasks]
        kin = dict(M=M, g=g, frames=frames)
    M = kin["M"]
    frames = list(kin["frames"])
    if pert is not None:
        M = M + pert["M"]
        dq = dq + pert["dq"]
        frames = [None if f is None else (f[0], f[1] + pert["x"][t], f[2] + pert["R"][t]) for t, f in enumerate(frames)]
        if "sf" in pert:
            goals = [g if pert["sf"][t] is None else dict(g, sf=M_(g["sf"]) + pert["sf"][t], sm=M_(g["sm"]) + pert["sm"][t])
                     for t, g in enumerate(goals)]
        for t, d in enumerate(pert.get("integ", [])):
            state[t]["integ"] = state[t]["integ"] + d
    Minv = inv(M)
    MiB = {}
    n = model.dof
    N_prec = eye(n)
    info, mods = [], []
    for ti, t in enumerate(tasks):
        out = {}
        thr = t["bie"]
        if thr not in MiB:
            MiB[thr] = bie_minv(M, thr)
        if t["kind"] == "mft":
            Jw, x, R = frames[ti]
            p = None if pert is None else dict(Jp=pert["Jp"][ti])
            unpert = kin["frames"][ti]
            m = _mft_update(model, t, state[ti], q, M, Minv, MiB[thr], Jw, N_prec, (unpert[1], unpert[2]), p,
                            None if types_override is None else types_override[ti], out)
        else:
            m = _jt_update(t, M, Minv, MiB[thr], N_prec, out)
        N_prec = m["N_total"]
        mods.append(m)
        info.append(out)
    tau = zeros(n)
    for ti, t in enumerate(tasks):
        if t["kind"] == "mft":
            Jw, x, R = frames[ti]
            tt = _mft_torques(model, t, state[ti], mods[ti], q, dq, x, R, goals[ti], info[ti])
        else:
            tt = _jt_torques(t, state[ti], mods[ti], q, dq, Minv, tau, goals[ti], info[ti])
        tau = tau + tt
    if gravity_comp:
        tau = tau + kin["g"]
    return tau, info, kin


def _sym_dir(rng, n):
    A = rng.standard_normal((n, n))
    return A + A.T


def perturbation(rng, kin, tasks, dq, Jps):
    """one seeded random direction: every model quantity moved normwise by eps times its own norm"""

    def scaled(d, ref):
        d = M_(d)
        return d * (mpf(EPS) * norm_fro(ref) / norm_fro(d))

    n = kin["M"].shape[0]
    p = dict(M=scaled(_sym_dir(rng, n), kin["M"]), dq=scaled(rng.standard_normal(n), M_(dq)) if np.any(dq) else zeros(n),
             Jp=[], x=[], R=[])
    for t, f in enumerate(kin["frames"]):
        if f is None:
            p["Jp"].append(None), p["x"].append(None), p["R"].append(None)
            continue
        p["Jp"].append(scaled(rng.standard_normal((6, n)), Jps[t]))
        p["x"].append(scaled(rng.standard_normal(3), f[1]))
        p["R"].append(scaled(rng.standard_normal((3, 3)), f[2]))
    return p


def perturbation_carried(rng, tasks, state, goals):
    """the same for what a tick carries besides the model: the sensed wrench (force and moment each by eps times its
    norm) and the integrators (position, orientation, force, moment, and a JointTask's, each by eps times its norm).
    Drawn from a generator of its own, so the directions of perturbation() are what they were before it existed"""

    def scaled(ref):
        ref = M_(ref)
        d = M_(rng.standard_normal(len(ref)))
        nr = norm_fro(ref)
        return d * (mpf(EPS) * nr / norm_fro(d)) if nr > 0 else zeros(len(ref))

    p = dict(sf=[], sm=[], integ=[])
    for t, g, st in zip(tasks, goals, state):
        has = t["kind"] == "mft" and "sf" in g
        p["sf"].append(scaled(g["sf"]) if has else None)
        p["sm"].append(scaled(g["sm"]) if has else None)
        i = st["integ"]
        p["integ"].append(np.concatenate([scaled(i[k: k + 3]) for k in range(0, 12, 3)]) if t["kind"] == "mft" else scaled(i))
    return p


INTEG_GROUPS = ("pos", "ori", "force", "moment", "jt")


def integ_groups(tasks, info):
    """the integrators after a tick, by group: the MotionForceTask's four and all JointTasks' together"""
    (mft,) = [i["integ"] for t, i in zip(tasks, info) if t["kind"] == "mft" and "integ" in i] or [zeros(12)]
    jt = [i["integ"] for t, i in zip(tasks, info) if t["kind"] == "jt" and "integ" in i]
    return [mft[0:3], mft[3:6], mft[6:9], mft[9:12], np.concatenate(jt) if jt else zeros(0)]


def kappa_emp(model, tasks, state_before, q, dq, goals, tau, info, kin, seed, dirs=16, gravity_comp=False, integ=False):
    """max over `dirs` seeded directions of ||dtau||_inf / (eps max(||tau||_inf, 1)): the error one ulp of noise in M,
    J N_prec, x / R, dq, the sensed wrench and the carried integrators causes, the classification held at the
    unperturbed decisions.
    integ: returns (kappa, kappa_integ), kappa_integ per group of INTEG_GROUPS the same for the integrators after the
    tick, plus the one rounding of storing them: (max ||d integ||_inf + eps ||integ||_inf) / (eps max(||integ||_inf, 1))"""
    rng = np.random.default_rng(seed)
    rng_c = np.random.default_rng([977] + list(np.atleast_1d(seed)))
    Jps = [i.get("Jp") for i in info]
    types = [None if i is None or "types" not in i else i["types"] for i in info]
    worst = mpf(0)
    groups = integ_groups(tasks, info)
    worst_i = [mpf(0)] * len(groups)
    for _ in range(dirs):
        st = copy.deepcopy(state_before)
        p = perturbation(rng, kin, tasks, dq, Jps)
        p.update(perturbation_carried(rng_c, tasks, st, goals))
        tp, ip, _ = tick(model, tasks, st, q, dq, goals, pert=p, types_override=types, kin=kin, gravity_comp=gravity_comp)
        worst = max(worst, norm_inf(tp - tau))
        worst_i = [max(w, norm_inf(a - b)) if len(a) else w for w, a, b in zip(worst_i, integ_groups(tasks, ip), groups)]
    kap = float(worst / (mpf(EPS) * max(norm_inf(tau), mpf(1))))
    if not integ:
        return kap
    return kap, [float((w + mpf(EPS) * norm_inf(g)) / (mpf(EPS) * max(norm_inf(g), mpf(1)))) if len(g) else 0.0
                 for w, g in zip(worst_i, groups)]


# ---- rigid-body dynamics: the simulation harness (csrc/sai2b_sim.hip) ----

GRAVITY = (0, 0, -9.81)


def _stencil(f, dps, second=False):
    """df/dt at t = 0 (and d^2f/dt^2 when second; f returns a flat object array): five-point central differences,
    evaluated at the extra precision that puts their truncation (h^4) and their cancellation both far below 10^-dps"""
    with mp.workdps(dps * 2 + 20):
        h = mpf(10) ** -(dps // 4 + 4)
        fm2, fm1, fp1, fp2 = f(-2 * h), f(-h), f(h), f(2 * h)
        d1 = (fm2 - 8 * fm1 + 8 * fp1 - fp2) / (12 * h)
        d2 = (-fm2 + 16 * fm1 - 30 * f(mpf(0)) + 16 * fp1 - fp2) / (12 * h * h) if second else None
    rnd = lambda d: np.array([+x for x in d], dtype=object)  # rounded to the working precision
    return (rnd(d1), rnd(d2)) if second else rnd(d1)


def _bodies(model, q):
    """per body hanging on a moving joint: (mass, COM Jacobian 6 x n, world inertia about the COM)"""
    pos, jinfo = model.poses(q)
    out = []
    for name, body in model.links.items():
        if body is None or pos[name][2] < 0:
            continue
        J, _, R = model.jacobian(pos, jinfo, name, M_(body["com"]))
        Ro = R @ _rpy([mpf(x) for x in body["rpy"]])
        out.append((name, mpf(body["m"]), J, Ro @ M_(body["I"]) @ Ro.T))
    return out


def _body_motion(model, q, v):
    """f(t) along q + t v: every body's COM position and angular velocity (with velocity v) stacked, flat"""

    def f(t):
        qt = q + t * v
        pos, jinfo = model.poses(qt)
        parts = []
        for name, body in model.links.items():
            if body is None or pos[name][2] < 0:
                continue
            R, p, mv = pos[name]
            w = zeros(3)
            for k in range(mv + 1):
                if jinfo[k][2] != "prismatic":
                    w = w + jinfo[k][0] * v[k]
            parts += list(p + R @ M_(body["com"])) + list(w)
        return np.array(parts, dtype=object)

    return f


def bias_terms(model, q, dq, gravity=None, parts=None):
    """b = sum_k Jv_k^T m_k a_k + Jw_k^T (I_k al_k + w_k x I_k w_k) - m_k Jv_k^T gravity, with a_k, al_k the COM and
    angular accelerations of body k at qdd = 0 (derivatives of the body poses along q + t dq). Returns (b, beta):
    beta[i] = the sum of the absolute values of the products b[i] is summed from (the forward-error scale).
    parts: a list, per body and force at its COM appended (index of the body, the force)"""
    q, dq = M_(q), M_(dq)
    n = model.dof
    dps = mp.dps
    bodies = _bodies(model, q)
    d1, d2 = _stencil(_body_motion(model, q, dq), dps, second=True)
    acc, alpha = d2.reshape(-1, 6)[:, :3], d1.reshape(-1, 6)[:, 3:]
    if "pris_coriolis_half" in HOOKS:  # the part of a_k bilinear in revolute and prismatic velocities, halved
        pris = np.array([j["type"] == "prismatic" for j in model.moving])
        vr, vp = dq.copy(), dq.copy()
        vr[pris], vp[~pris] = mpf(0), mpf(0)
        ar = _stencil(_body_motion(model, q, vr), dps, second=True)[1].reshape(-1, 6)[:, :3]
        ap = _stencil(_body_motion(model, q, vp), dps, second=True)[1].reshape(-1, 6)[:, :3]
        acc = ar + ap + (acc - ar - ap) / 2
    b, beta = zeros(n), zeros(n)
    gr = M_(GRAVITY if gravity is None else gravity) if gravity is not False else zeros(3)
    for k, (_, m, J, Iw) in enumerate(bodies):
        Jv, Jw = J[:3], J[3:]
        w = Jw @ dq
        Ia = Iw @ alpha[k]
        gyro = _cross(w, Iw @ w) if "no_gyroscopic" not in HOOKS else zeros(3)
        for vec, Jx in ((m * acc[k], Jv), (Ia, Jw), (gyro, Jw), (-m * gr, Jv)):
            b += Jx.T @ vec
            beta += np.abs(Jx).T @ np.abs(vec)
            if parts is not None and Jx is Jv:
                parts.append((k, vec))
    return b, beta


def bias(model, q, dq, gravity=None):
    """b = C(q, dq) dq + g(q); gravity None: the model's (0, 0, -9.81), False: none"""
    return bias_terms(model, q, dq, gravity)[0]


def bias_lagrange(model, q, dq, gravity=None):
    """the Lagrangian form b_i = sum_jk dM_ij/dq_k dq_k dq_j - 1/2 dq^T dM/dq_i dq + g_i, derivatives of M"""
    q, dq = M_(q), M_(dq)
    n = model.dof
    dps = mp.dps
    Mf = lambda v: (lambda t: model.dynamics(q + t * v)[2].ravel())
    Mdot = _stencil(Mf(dq), dps).reshape(n, n)
    b = Mdot @ dq
    for i in range(n):
        e = zeros(n)
        e[i] = mpf(1)
        b[i] -= dq @ _stencil(Mf(e), dps).reshape(n, n) @ dq / 2
    if gravity is not False:
        b = b + model.dynamics(q, GRAVITY if gravity is None else gravity)[3]
    return b


def solve(M, r):
    return np.array(list(mp.lu_solve(mp.matrix(M.tolist()), mp.matrix(list(r)))), dtype=object)


def sim_step(model, q, dq, tau, dt, substeps, gravity, info=None):
    """one control period of csrc/sai2b_sim.hip: tau held, `substeps` semi-implicit Euler steps of h = dt / substeps,
    dq += h M^-1 (tau - b), q += h dq (b with g when gravity). Returns (q, dq). info: a list, per step appended
    cond_2(M), ||M^-1||_2, ||M^-1 (tau - b)||_inf and ||beta||_inf of the bias"""
    q, dq, tau = M_(q), M_(dq), M_(tau)
    h = mpf(dt) / substeps
    for _ in range(substeps):
        M = model.dynamics(q)[2]
        b, beta = bias_terms(model, q, dq, None if gravity else False)
        x = solve(M, tau - b)
        if info is not None:
            with mp.workdps(20):
                ev = mp.eigsy(mp.matrix(M.tolist()), eigvals_only=True)
                lo, hi = min(ev), max(ev)
                info.append(dict(cond=float(hi / lo), minv=float(1 / lo), x=float(norm_inf(x)), beta=float(norm_inf(beta))))
        dq_old = dq
        dq = dq + h * x
        q = q + h * (dq_old if "explicit_euler" in HOOKS else dq)
    return q, dq


# ---- the simulated plant: contact, joint dynamics, external wrench (DESIGN "Contact in the simulated plant", "Joint
# dynamics in the simulated plant", "External wrench on a link"), written from those laws ----
# Point Jacobians are formed explicitly (Model.jacobian) and the implicit system is solved by LU. The inputs are dicts:
#   joint    rows [6][n] (armature, damping, friction, torque limit, lower, upper), k, c, e [n]
#   contact  link (URDF name), points [K][3] (URDF link frame), rows [9] (p0, n, k, d, mu), v_eps, sensor (a task, or None)
#   wrench   link, point (URDF link frame), frame ("world" | "link": components in the URDF link frame), rows [7]
#            (F, M, steps on entry of the call), sensor (a task, or None)
#   a task   link, point, frot (Model.frame), sensor_rot [9], sensor_pos [3]
#   payload  the Model of the same robot carrying the payload's body: M and b are its
# HOOKS plants errors for tests/test_hp_plant.py: diss_explicit, rhs_no_armature, upper_stop_minus, contact_outboard,
# contact_pris_as_rev, friction_along_v, moment_about_link_origin, couple_on_prismatic, wrench_frame_period_start,
# wrench_never_expires, shared_sensor_no_wrench_moment.

class Noise:
    """seeded relative perturbations of size eps (times `scale`), for the scales of tests/golden/hp_plant.npz: what
    roundings of the working precision of a float64 implementation do to the plant's answer"""

    def __init__(self, seed, scale=1.0):
        self.rng = np.random.default_rng(seed)
        self.e = mpf(EPS) * scale

    def u(self, *shape):
        return M_(self.rng.uniform(-1, 1, shape))

    def rel(self, v):
        """every component by eps of itself"""
        v = np.asarray(v, dtype=object)
        return v * (1 + self.e * self.u(*v.shape))

    def add(self, v, s):
        """every component by eps s (s: a number or an array of v's shape)"""
        v = np.asarray(v, dtype=object)
        return v + self.e * s * self.u(*v.shape)

    def sym(self, A):
        """a symmetric matrix by eps of its Frobenius norm"""
        d = self.u(*A.shape)
        return A + self.e * norm_fro(A) * (d + d.T) / 2


def _pmax(a, b):
    return a if a > b else b


def wrench_active(steps):
    """steps > 0 or steps < 0 on entry (a NaN is inactive)"""
    s = mpf(steps)
    return bool(s > 0 or s < 0)


def wrench_countdown(steps):
    """what a call leaves in the row: steps > 0 ? max(steps - 1, 0) : steps (a float)"""
    s = float(steps)
    if "wrench_never_expires" in HOOKS:
        return s
    return max(s - 1.0, 0.0) if s > 0 else s


def _point_jacobian(model, pos, jinfo, link, point, outboard=False):
    """(Jv 3 x n, Jw 3 x n, x) of a point of a link; outboard: the joints past the link counted as if they moved it"""
    J, x, _ = model.jacobian(pos, jinfo, link, M_(point))
    if outboard:
        for k in range(pos[link][2] + 1, model.dof):
            aw, o, typ = jinfo[k]
            J[:3, k] = aw if typ == "prismatic" else _cross(aw, x - o)
    return J[:3], J[3:], x


def _contact_eval(model, pos, jinfo, dq, contact, nz):
    """per point (x, F, delta, f_n) and tc = sum J_k^T F_k with its sum of absolute products"""
    rows = M_(contact["rows"])
    p0, nrm, k, d, mu = rows[0:3], rows[3:6], rows[6], rows[7], rows[8]
    ve = mpf(contact["v_eps"])
    n = model.dof
    pts, tc, mag = [], zeros(n), zeros(n)
    for c in contact["points"]:
        Jv, _, x = _point_jacobian(model, pos, jinfo, contact["link"], c, "contact_outboard" in HOOKS)
        if nz is not None:  # the point and its lever arms carry the rounding of world positions
            far = norm_inf(x)
            x = nz.add(x, far)
            for i in range(n):
                if jinfo[i][2] != "prismatic" and any(Jv[:, i]):
                    Jv[:, i] = nz.add(Jv[:, i], far)
            Jv = nz.rel(Jv)
        v = Jv @ dq
        if nz is not None:
            v = nz.add(v, np.abs(Jv) @ np.abs(dq))
        delta = nrm @ (p0 - x)
        vn = nrm @ v
        fn = _pmax(mpf(0), k * _pmax(mpf(0), delta) * (1 - d * vn))
        vt = v if "friction_along_v" in HOOKS else v - vn * nrm
        F = fn * nrm - mu * fn * vt / mp.sqrt(vt @ vt + ve * ve)
        if nz is not None:
            F = nz.rel(F)
        Jt = Jv
        if "contact_pris_as_rev" in HOOKS:
            Jt = Jv.copy()
            for i in range(pos[contact["link"]][2] + 1):
                if jinfo[i][2] == "prismatic":
                    Jt[:, i] = _cross(jinfo[i][0], x - jinfo[i][1])
        tc = tc + Jt.T @ F
        mag = mag + np.abs(Jt).T @ np.abs(F)
        pts.append((x, F, delta, fn))
    if nz is not None:
        tc = nz.add(tc, mag)
    return pts, tc


def _wrench_eval(model, pos, jinfo, wrench, active, nz, R_first=None):
    """x, F_w, M_w, tx of an active robot (zeros of an inactive one)"""
    n = model.dof
    link = wrench["link"]
    Jv, Jw, x = _point_jacobian(model, pos, jinfo, link, wrench["point"])
    if not active:
        return x, zeros(3), zeros(3), zeros(n)
    rows = M_(wrench["rows"])
    F, Mo = rows[0:3], rows[3:6]
    if wrench["frame"] == "link":
        Rl = pos[link][0] if R_first is None else R_first
        if nz is not None:
            Rl = nz.add(Rl, 1)
        F, Mo = Rl @ F, Rl @ Mo
    if nz is not None:
        far = norm_inf(x)
        x = nz.add(x, far)
        for i in range(n):
            if jinfo[i][2] != "prismatic" and any(Jv[:, i]):
                Jv[:, i] = nz.add(Jv[:, i], far)
        F, Mo = nz.rel(F), nz.rel(Mo)
    tx = Jv.T @ F + Jw.T @ Mo
    if "couple_on_prismatic" in HOOKS:
        for i in range(pos[link][2] + 1):
            if jinfo[i][2] == "prismatic":
                tx[i] += jinfo[i][0] @ Mo
    if nz is not None:
        tx = nz.add(tx, np.abs(Jv).T @ np.abs(F) + np.abs(Jw).T @ np.abs(Mo))
    return x, F, Mo, tx


def _joint_terms(q, dq, tau, joint, nz):
    """ts, sl, su, g of the law"""
    a, d, f, t, lo, hi = (M_(r) for r in joint["rows"])
    k, c, e = M_(joint["k"]), M_(joint["c"]), M_(joint["e"])
    n = len(q)
    z = mpf(0)
    ts = np.array([min(max(tau[i], -t[i]), t[i]) for i in range(n)], dtype=object)
    sl = np.array([_pmax(z, k[i] * _pmax(z, lo[i] - q[i]) * (1 - c[i] * dq[i])) for i in range(n)], dtype=object)
    sgn = -1 if "upper_stop_minus" in HOOKS else 1
    su = np.array([_pmax(z, k[i] * _pmax(z, q[i] - hi[i]) * (1 + sgn * c[i] * dq[i])) for i in range(n)], dtype=object)
    g = np.array([d[i] + f[i] / mp.sqrt(dq[i] * dq[i] + e[i] * e[i]) for i in range(n)], dtype=object)
    if nz is not None:
        sl, su, g = nz.rel(sl), nz.rel(su), nz.rel(g)
    return a, ts, sl, su, g


def _lever_noise(dyn, q, parts, nz):
    """what the rounding of the bodies' world positions does to M and b: the COM of body k by eps of its own size, and
    with it every lever arm of a revolute column of its Jacobian, as for the contact points. -> dM, db"""
    pos, jinfo = dyn.poses(q)
    n = dyn.dof
    dM, db = zeros(n, n), zeros(n)
    k = 0
    for name, body in dyn.links.items():
        if body is None or pos[name][2] < 0:
            continue
        J, x, _ = dyn.jacobian(pos, jinfo, name, M_(body["com"]))
        far, m = norm_inf(x), mpf(body["m"])
        dJ = zeros(3, n)
        for i in range(pos[name][2] + 1):
            if jinfo[i][2] != "prismatic":
                dJ[:, i] = nz.e * far * nz.u(3)
        dM = dM + m * (dJ.T @ J[:3] + J[:3].T @ dJ)
        for kk, vec in parts:
            if kk == k:
                db = db + dJ.T @ vec
        k += 1
    return dM, db


def plant_step(model, q, dq, tau, dt, substeps, gravity, joint=None, contact=None, wrench=None, payload=None, info=None):
    """one control period of the simulated plant: tau held, `substeps` steps of h = dt / substeps, each from the state
    at its start: without joint dynamics dq+ = dq + h M^-1 (tau + tc + tx - b), with them
    (M + diag(a) + h diag(g)) dq+ = (M + diag(a)) dq + h (ts + sl - su + tc + tx - b); q+ = q + h dq+.
    The wrench acts when its steps row is > 0 or < 0 on entry; the countdown is the caller's (wrench_countdown).
    info: a dict; info["noise"], a Noise, perturbs every quantity a float64 implementation rounds. Returns (q, dq)."""
    q, dq, tau = M_(q), M_(dq), M_(tau)
    n = model.dof
    dyn = model if payload is None else payload
    nz = None if info is None else info.get("noise")
    h = mpf(dt) / substeps
    active = wrench is not None and wrench_active(wrench["rows"][6])
    R_first = None
    for _ in range(substeps):
        if nz is not None:
            q, dq = nz.rel(q), nz.rel(dq)
        pos, jinfo = model.poses(q)
        M = dyn.dynamics(q)[2]
        parts = None if nz is None else []
        b, beta = bias_terms(dyn, q, dq, None if gravity else False, parts=parts)
        if nz is not None:
            dM, db = _lever_noise(dyn, q, parts, nz)
            M, b = nz.sym(M) + dM, nz.add(b, beta) + db
        tc = _contact_eval(model, pos, jinfo, dq, contact, nz)[1] if contact is not None else zeros(n)
        tx = zeros(n)
        if wrench is not None:
            if "wrench_frame_period_start" in HOOKS and R_first is None:
                R_first = pos[wrench["link"]][0]
            tx = _wrench_eval(model, pos, jinfo, wrench, active, nz, R_first)[3]
        if joint is None:
            r = tau + tc + tx - b
            if nz is not None:
                r = nz.add(r, np.abs(tau) + np.abs(tc) + np.abs(tx) + np.abs(b))
            dq = dq + h * solve(M, r)
        else:
            a, ts, sl, su, g = _joint_terms(q, dq, tau, joint, nz)
            Ma = M + np.diag(a)
            Mr = M if "rhs_no_armature" in HOOKS else Ma
            r = ts + sl - su + tc + tx - b
            mag = np.abs(Mr) @ np.abs(dq) + h * (np.abs(ts) + np.abs(sl) + np.abs(su) + np.abs(tc) + np.abs(tx) + np.abs(b))
            if "diss_explicit" in HOOKS:
                A, rhs = Ma, Mr @ dq + h * (r - g * dq)
            else:
                A, rhs = Ma + h * np.diag(g), Mr @ dq + h * r
            if nz is not None:
                A, rhs = nz.sym(A), nz.add(rhs, mag)
            dq = solve(A, rhs)
        q = q + h * dq
    return q, dq


def _sensor_frame(model, pos, jinfo, task, nz):
    """x_c, o_s, R_s of a task's sensor"""
    _, xc, Rc = model.frame(pos, jinfo, task)
    if nz is not None:
        xc, Rc = nz.add(xc, norm_inf(xc)), nz.add(Rc, 1)
    return xc, xc + Rc @ M_(task["sensor_pos"]), Rc @ M_(np.asarray(task["sensor_rot"]).reshape(3, 3))


def plant_report(model, q, dq, tau, joint=None, contact=None, wrench=None, info=None):
    """what the kernels store after the last substep of a call, from the state (q, dq) it ended in (tau: the torques held
    in it, wrench["rows"][6]: the steps row on its entry). A dict of float-able mpf arrays:
      contact   depth, normal_force [K], wrench_world [6] (sum F_k, sum (x_k - x_c) x F_k; x_c: the control point of the
                contact's sensor task, the link origin without one), touching
      joint     applied_torque, stop_torque, dissipative_torque [n], saturated, at_stop
      wrench    ext_wrench [6] (F_w, M_w), ext_torque [n], steps (counted down), pushed
      sensed    {id(task) -> [6]}: f_s = R_s^T (-F), m_s = R_s^T (-sum moments about o_s); one task shared by contact and
                wrench reads the sum"""
    q, dq, tau = M_(q), M_(dq), M_(tau)
    nz = None if info is None else info.get("noise")
    pos, jinfo = model.poses(q)
    out, sensed = {}, {}
    if contact is not None:
        pts, _ = _contact_eval(model, pos, jinfo, dq, contact, nz)
        task = contact.get("sensor")
        if task is not None:
            xc, os_, Rs = _sensor_frame(model, pos, jinfo, task, nz)
        xo = pos[contact["link"]][1]
        about = xo if task is None or "moment_about_link_origin" in HOOKS else xc
        Ft = sum((p[1] for p in pts), zeros(3))
        out.update(depth=np.array([p[2] for p in pts], dtype=object), normal_force=np.array([p[3] for p in pts], dtype=object),
                   wrench_world=np.concatenate([Ft, sum((_cross(p[0] - about, p[1]) for p in pts), zeros(3))]),
                   touching=any(p[3] > 0 for p in pts))
        if task is not None:
            sensed[id(task)] = [task, Rs, -Ft, -sum((_cross(p[0] - os_, p[1]) for p in pts), zeros(3))]
    if joint is not None:
        a, ts, sl, su, g = _joint_terms(q, dq, tau, joint, nz)
        t = M_(joint["rows"][3])
        out.update(applied_torque=ts, stop_torque=sl - su, dissipative_torque=-g * dq,
                   saturated=any(abs(tau[i]) > t[i] for i in range(len(q))), at_stop=any(x != 0 for x in sl - su))
    if wrench is not None:
        steps = wrench["rows"][6]
        active = wrench_active(steps)
        x, Fw, Mw, tx = _wrench_eval(model, pos, jinfo, wrench, active, nz)
        out.update(ext_wrench=np.concatenate([Fw, Mw]), ext_torque=tx, steps=wrench_countdown(steps),
                   pushed=active and any(float(v) != 0 for v in wrench["rows"][0:6]))
        task = wrench.get("sensor")
        if task is not None:
            _, os_, Rs = _sensor_frame(model, pos, jinfo, task, nz)
            f, m = -Fw, -(Mw + _cross(x - os_, Fw))
            if id(task) in sensed:
                sensed[id(task)][2] = sensed[id(task)][2] + f
                if "shared_sensor_no_wrench_moment" not in HOOKS:
                    sensed[id(task)][3] = sensed[id(task)][3] + m
            else:
                sensed[id(task)] = [task, Rs, f, m]
    out["sensed"] = {k: np.concatenate([Rs.T @ f, Rs.T @ m]) for k, (_, Rs, f, m) in sensed.items()}
    return out

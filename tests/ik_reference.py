"""The inverse-kinematics law (include/sai2b.h "inverse kinematics") restated in numpy, vectorised over robots (test
infrastructure). The chain is walked here, from the URDF text as tests/urdf_np.Chain parses it: joint origin, then a Rodrigues
rotation about (a translation along) the joint's own <axis>, fixed joints included. Nothing of the product's header, model code
or folded z axes is used, and nothing of the oracle. The GPU tests (tests/test_gpu_ik.py) and the CPU run of the law's own
header (tests/test_ik_law.py) are held to this file; tests/test_ik_reference.py pins it.

The control frame is (URDF link name, position in that link, rotation in that link). The product takes a moving-link index and
a frame in the MODEL's link frame: `product_frame` carries it over with the loader's own sai2b_urdf_resolve_frame.

SEPARATION. Every decision of the law that hangs on a comparison is recorded with its relative distance to its threshold:
accept / reject (|E' - E| / E, unless q' is q itself), the step_max test, every clamp of a step (|q_i + d_i - limit| /
max(1, |limit|)), both convergence tests and the comparison of two starts' candidates. `sep` is a robot's smallest over every
decision that can reach an output: the convergence tests and the candidates' comparisons of every start, and the path decisions
(step_max, clamps, accept / reject) of the start that produced q_out and of the last start (whose mu is a status row). The path
of a start that ends unconverged and loses reaches no output: its iterations count max_iterations whatever it decided. A
comparison of implementations value by value leaves out the robots with sep < 1e-9 (SEPARATION), whose outputs may legitimately
differ.
A relative distance is never taken finer than the compared quantity is known: the components of e are differences of numbers of
order 1 and carry an absolute rounding error of order 1e-15 however small they are, so E = |W e|^2 is uncertain by about
1e-15 sqrt(E) and the error norms by 1e-15. The scale of an E comparison is therefore E + 1e-3 sqrt(E) (at 1e-9: a thousand such
roundings), that of a convergence test its tolerance + 1e-4 (at 1e-9: 1e-13).

Philox: tests/hardware_reference.py's, through tests/reset_sampler_reference.uniforms, on stream 11."""
import numpy as np

import reset_sampler_reference as rr
import urdf_np

STREAM = 11
CONVERGED, EXHAUSTED, AT_LIMIT, NONFINITE = 1, 2, 4, 8
SEPARATION = 1e-9
DEFAULTS = dict(axes=63, rot_length=0.25, max_iterations=40, restarts=0, tol_pos=1e-6, tol_rot=1e-6, mu0=1e-2, mu_min=1e-9, mu_max=1e3, mu_down=0.25,
                mu_up=8.0, step_max=0.5, use_limits=True, limit_margin=0.0, rest_weight=0.0, seed=0, first_robot=0, draw_id=0)


def rotation_exp(r):
    """r [B][3] -> R [B][3][3], Rodrigues"""
    r = np.asarray(r, dtype=float)
    th = np.linalg.norm(r, axis=1)
    a = r / np.where(th > 0, th, 1.0)[:, None]
    K = np.zeros((len(r), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    return np.eye(3) + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def rotation_log(D):
    """D [B][3][3] -> r [B][3], the law's logarithm with its two branches (c >= 0: from the skew part; c < 0: axis from the
    symmetric part)"""
    c = np.clip(0.5 * (np.trace(D, axis1=1, axis2=2) - 1.0), -1.0, 1.0)
    v = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)
    s = np.linalg.norm(v, axis=1)
    th = np.arctan2(s, c)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(s < 1e-12, 1.0, th / np.where(s > 0, s, 1.0))
        small = f[:, None] * v
        M = 0.5 * (D + np.transpose(D, (0, 2, 1))) - c[:, None, None] * np.eye(3)
        dg = np.stack([M[:, 0, 0], M[:, 1, 1], M[:, 2, 2]], axis=1)
        k = np.argmax(dg, axis=1)  # the first largest
        rows = np.arange(len(D))
        a = M[rows, :, k] / np.sqrt((1.0 - c) * dg[rows, k])[:, None]
        a = np.where((np.sum(a * v, axis=1) < 0)[:, None], -a, a)
        large = th[:, None] * a
    return np.where((c >= 0)[:, None], small, large)


class IkReference:
    def __init__(self, urdf_text, link, frame_pos=(0.0, 0.0, 0.0), frame_rot=None, lower=None, upper=None, **cfg):
        """link: URDF link name; lower, upper [dof]: the model's joint limits; cfg: DEFAULTS' keys"""
        ch = urdf_np.Chain(urdf_text, is_file=False)
        self.dof = ch.dof
        # the joints from the root to the link, in order
        by_child = {j["child"]: j for j in ch.joints}
        path, cur = [], link
        while cur != ch.root:
            path.append(by_child[cur])
            cur = path[-1]["parent"]
        self.path = path[::-1]
        self.index = [ch.moving.index(j) if j["type"] != "fixed" else -1 for j in self.path]
        self.fp = np.asarray(frame_pos, dtype=float)
        self.fr = np.eye(3) if frame_rot is None else np.asarray(frame_rot, dtype=float).reshape(3, 3)
        unknown = set(cfg) - set(DEFAULTS)
        assert not unknown, unknown
        self.cfg = dict(DEFAULTS, **cfg)
        c = self.cfg
        lower, upper = np.asarray(lower, dtype=float), np.asarray(upper, dtype=float)
        self.lo = lower + c["limit_margin"] if c["use_limits"] else np.full(self.dof, -np.inf)
        self.hi = upper - c["limit_margin"] if c["use_limits"] else np.full(self.dof, np.inf)
        on = np.array([(c["axes"] >> a) & 1 for a in range(6)], dtype=float)
        self.sel = on
        self.w2 = on * np.array([1, 1, 1] + [c["rot_length"] ** 2] * 3)

    # ---- kinematics
    def fk(self, q, jac=False):
        """q [B][dof] -> x [B][3], R [B][3][3] of the control frame (and J [B][6][dof])"""
        B = q.shape[0]
        R, p = np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3))
        axes = []
        for j, k in zip(self.path, self.index):
            p = p + R @ j["xyz"]
            R = R @ j["R"]
            if k < 0:
                continue
            a = j["axis"] / np.linalg.norm(j["axis"])
            aw = R @ a
            if j["type"] == "prismatic":
                p = p + aw * q[:, k : k + 1]
            else:
                K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
                R = R @ (np.eye(3) + np.sin(q[:, k])[:, None, None] * K + (1 - np.cos(q[:, k]))[:, None, None] * (K @ K))
            axes.append((k, aw, p.copy(), j["type"]))
        x = p + R @ self.fp
        Rc = R @ self.fr
        if not jac:
            return x, Rc
        J = np.zeros((B, 6, self.dof))
        for k, aw, o, typ in axes:
            if typ == "prismatic":
                J[:, :3, k] = aw
            else:
                J[:, :3, k] = np.cross(aw, x - o)
                J[:, 3:, k] = aw
        return x, Rc, J

    def error(self, xg, Rg, x, R):
        """-> e [B][6] = (x_goal - x ; log(R_goal R^T))"""
        return np.concatenate([xg - x, rotation_log(Rg @ np.transpose(R, (0, 2, 1)))], axis=1)

    def norms(self, e):
        """-> E = |W e|^2, pos, rot: [B] each"""
        s = e * e
        return s @ self.w2, np.sqrt(s[:, :3] @ self.sel[:3]), np.sqrt(s[:, 3:] @ self.sel[3:])

    def clamp(self, q):
        return np.minimum(np.maximum(q, self.lo), self.hi)

    def restart_seed(self, n, robots):
        """start n >= 1 of the robots with these indices in their context -> q [len][dof]"""
        c = self.cfg
        robot = np.asarray(robots, dtype=np.uint64) + np.uint64(c["first_robot"])
        u = rr.uniforms(np.asarray(n), c["draw_id"], STREAM, robot, c["seed"], self.dof)
        return (self.lo[:, None] + (self.hi - self.lo)[:, None] * u).T

    def step(self, q, J, e, mu, rest=None):
        """the raw solve of one iteration -> d [B][dof] before scaling"""
        nu = self.cfg["rest_weight"] if rest is not None else 0.0
        JW = J * self.w2[None, :, None]
        H = np.transpose(J, (0, 2, 1)) @ JW + (mu + nu)[:, None, None] * np.eye(self.dof)
        g = np.einsum("brn,br->bn", JW, e)
        if rest is not None:
            g = g + nu * (rest - q)
        return np.linalg.solve(H, g[:, :, None])[:, :, 0]

    # ---- the law
    def solve(self, goal_rows, seed_rows, mask=None, track_sigma=False):
        """goal_rows [12 (+ dof)][B], seed_rows [dof][B], mask [B] or None -> dict: q [dof][B], status [5][B], flags [B] uint8 (0 for
        an unselected robot, whose q and status are NaN here), counts [4], sep [B], sigma_min [B] (track_sigma: the smallest singular
        value of W J over the accepted iterates), trace: per robot the list of E after every trip when B is small"""
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return self._solve(np.asarray(goal_rows, dtype=float), np.asarray(seed_rows, dtype=float), mask, track_sigma)

    def _solve(self, goal_rows, seed_rows, mask, track_sigma):
        c, n = self.cfg, self.dof
        B = seed_rows.shape[1]
        xg, Rg = goal_rows[:3].T.copy(), goal_rows[3:12].T.reshape(B, 3, 3).copy()
        rest = goal_rows[12 : 12 + n].T.copy() if c["rest_weight"] > 0 else None
        sel = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        finite = np.isfinite(goal_rows[:12]).all(axis=0) & np.isfinite(seed_rows).all(axis=0)
        if rest is not None:
            finite &= np.isfinite(rest).all(axis=1)
        nu = c["rest_weight"] if rest is not None else 0.0
        q = seed_rows.T.copy()
        x, R, J, e = np.zeros((B, 3)), np.zeros((B, 3, 3)), np.zeros((B, 6, n)), np.zeros((B, 6))
        E, mu = np.full(B, np.inf), np.full(B, c["mu0"])
        qb, bE, bp, br, bs = np.zeros((B, n)), np.full(B, np.inf), np.full(B, np.inf), np.full(B, np.inf), np.zeros(B, dtype=int)
        start, k, it = np.zeros(B, dtype=int), np.zeros(B, dtype=int), np.zeros(B, dtype=int)
        fresh, conv, active = np.ones(B, dtype=bool), np.zeros(B, dtype=bool), sel & finite
        smin = np.full(B, np.inf)
        # separation: of the path of the start under way (step_max, clamps, accept / reject), of the path of the start that gave
        # the best candidate, and of what ends a start or picks a candidate (convergence tests, the candidates' comparison)
        sep_path, sep_best, sep_ends = np.full(B, np.inf), np.full(B, np.inf), np.full(B, np.inf)

        def near(i, value, threshold, scale, where=None):
            where = sep_path if where is None else where
            with np.errstate(invalid="ignore", divide="ignore"):
                d = np.abs(value - threshold) / scale
            where[i] = np.fmin(where[i], d)

        while active.any():
            i = np.nonzero(active)[0]
            fr = fresh[i]
            qn = q[i].copy()
            # restarts: the drawn seeds
            for s in np.unique(start[i][fr & (start[i] > 0)]):
                w = fr & (start[i] == s)
                qn[w] = self.restart_seed(int(s), i[w])
            # steps
            d = self.step(q[i], J[i], e[i], mu[i], None if rest is None else rest[i])
            big = np.abs(d).max(axis=1)
            near(i[~fr], big[~fr], c["step_max"], c["step_max"])
            scale = np.where(big > c["step_max"], c["step_max"] / big, 1.0)
            stepped = q[i] + scale[:, None] * d
            if c["use_limits"]:
                for lim in (self.lo, self.hi):
                    dist = (np.abs(stepped - lim) / np.maximum(1.0, np.abs(lim))).min(axis=1)
                    near(i[~fr], dist[~fr], 0.0, 1.0)
            qn = self.clamp(np.where(fr[:, None], qn, stepped))
            xn, Rn, Jn = self.fk(qn, jac=True)
            en = self.error(xg[i], Rg[i], xn, Rn)
            En, _, _ = self.norms(en)
            # (a candidate that is the iterate itself, every joint held by its limit or the step below an ulp, is rejected by
            # construction: E' is E bit for bit in any implementation, and the comparison is strict)
            moved = ~fr & (qn != q[i]).any(axis=1)
            near(i[moved], En[moved], E[i][moved], E[i][moved] + 1e-3 * np.sqrt(E[i][moved]))
            acc = fr | (En < E[i])
            a = i[acc]
            q[a], x[a], R[a], J[a], e[a], E[a] = qn[acc], xn[acc], Rn[acc], Jn[acc], en[acc], En[acc]
            if track_sigma and len(a):
                sv = np.linalg.svd(J[a] * np.sqrt(self.w2)[None, :, None], compute_uv=False)
                smin[a] = np.fmin(smin[a], sv[:, : min(n, int((self.w2 > 0).sum()))].min(axis=1))
            nf = i[~fr]
            mu[nf] = np.where(acc[~fr], np.maximum(mu[nf] * c["mu_down"], c["mu_min"]), np.minimum(mu[nf] * c["mu_up"], c["mu_max"]))
            mu[i[fr]] = c["mu0"]
            k[nf] += 1
            it[nf] += 1
            fresh[i] = False
            _, ep, er = self.norms(e[i])
            if c["tol_pos"] > 0:
                near(i, ep, c["tol_pos"], c["tol_pos"] + 1e-4, sep_ends)
            if c["tol_rot"] > 0:
                near(i, er, c["tol_rot"], c["tol_rot"] + 1e-4, sep_ends)
            cv = (ep <= c["tol_pos"]) & (er <= c["tol_rot"])
            conv[i] = cv
            end = cv | (k[i] >= c["max_iterations"])
            better = end & (cv | (start[i] == 0) | (E[i] < bE[i]))
            rival = end & ~cv & (start[i] > 0)
            near(i[rival], E[i][rival], bE[i][rival], bE[i][rival] + 1e-3 * np.sqrt(bE[i][rival]), sep_ends)
            b = i[better]
            qb[b], bE[b], bp[b], br[b], bs[b] = q[b], E[b], ep[better], er[better], start[b]
            sep_best[b] = sep_path[b]
            stop = end & (cv | (start[i] >= c["restarts"]))
            active[i[stop]] = False
            again = i[end & ~stop]
            start[again] += 1
            k[again] = 0
            fresh[again] = True
            sep_path[again] = np.inf
        done = sel & finite
        flags = np.zeros(B, dtype=np.uint8)
        flags[done] = np.where(conv[done], CONVERGED, EXHAUSTED)
        if c["use_limits"]:
            flags[done & ((qb <= self.lo) | (qb >= self.hi)).any(axis=1)] |= AT_LIMIT
        flags[sel & ~finite] = NONFINITE
        q_out = np.where(done[:, None], qb, np.nan).T
        status = np.where(done[None, :], np.stack([bp, br, it.astype(float), bs.astype(float), mu]), np.nan)
        counts = [int(sel.sum()), int((done & conv).sum()), int((done & ~conv).sum()), int((sel & ~finite).sum())]
        # sep_path is now the last start's: its mu is a status row
        sep = np.fmin(np.fmin(sep_best, sep_ends), sep_path)
        return dict(q=np.ascontiguousarray(q_out), status=status, flags=flags, counts=counts, sep=sep, sigma_min=smin)

    def pose_error(self, goal_rows, q):
        """pos, rot [B] of q [dof][B] against the goals, by this file's own forward kinematics"""
        B = q.shape[1]
        x, R = self.fk(np.asarray(q, dtype=float).T)
        e = self.error(goal_rows[:3].T, goal_rows[3:12].T.reshape(B, 3, 3), x, R)
        _, ep, er = self.norms(e)
        return ep, er

    def goal_rows(self, q):
        """the pose rows [12][B] of the control frame at q [dof][B]"""
        x, R = self.fk(np.asarray(q, dtype=float).T)
        return np.ascontiguousarray(np.concatenate([x, R.reshape(len(x), 9)], axis=1).T)


def product_frame(pkg, links, link, frame_pos=(0.0, 0.0, 0.0), frame_rot=None):
    """(moving link index, frame_pos, frame_rot) in the model's link frame, for motion_force_task_config"""
    return pkg.resolve_link_frame(links, link, frame_pos, frame_rot)

"""The collision-proximity law (include/sai2b.h "collision proximity") restated in numpy on tests/urdf_np.Chain, an independent
reading of the URDF: `poses` gives the link frames the sphere centres hang on, `jacobian` the gradients. Nothing of the product or
the oracle is used. The GPU tests (tests/test_gpu_collision.py) and the CPU run of the law's own header
(tests/test_collision_law.py) are held to this file; tests/test_collision_reference.py pins it.

A sphere is (URDF link name or None for the world, centre in that link's frame, radius). The product takes a moving-link index
and a centre in the MODEL's link frame (the joint axis folded onto z): `product_spheres` carries the centres over with the
loader's own sai2b_urdf_resolve_frame, as tests/test_contact_reference.py does for contact points.

One robot at a time, in plain loops that read like the specification: p outer / k inner, o outer / k inner, i outer / j inner,
the first strict minimum wins, a NaN loses every comparison."""
import numpy as np

import urdf_np

CATEGORIES = ("plane", "obstacle", "self")
FLAG_PLANE, FLAG_OBSTACLE, FLAG_SELF, FLAG_NONFINITE = 1, 2, 4, 8


def default_masks(links):
    """env_mask: every sphere on a moving link; pair_mask[i] bit j (i < j): the links differ by at least 2, -1 counting as a link"""
    n = len(links)
    env = sum(1 << k for k in range(n) if links[k] >= 0)
    pairs = [0] * 16
    for i in range(n):
        for j in range(i + 1, n):
            if abs(int(links[i]) - int(links[j])) >= 2:
                pairs[i] |= 1 << j
    return env, pairs


class CollisionReference:
    def __init__(self, urdf_text, spheres, n_planes=0, n_obstacles=0, env_mask=None, pair_mask=None, margins=(0.0, 0.0, 0.0), base=None):
        """spheres: [(link name | None, centre [3], radius)]; base: (pos [3], R [3][3]) of the robot's root in the world or None"""
        self.chain = urdf_np.Chain(urdf_text, is_file=False)
        self.dof = self.chain.dof
        # a robot's frames are needed for its centres and again inside every `jacobian`: the chain's own `poses`, remembered for
        # the last q
        poses, last = self.chain.poses, [None, None]

        def remembered(q):
            key = np.asarray(q, dtype=float).tobytes()
            if last[0] != key:
                last[0], last[1] = key, poses(q)
            return last[1]

        self.chain.poses = remembered
        self.spheres = [(name, np.asarray(c, dtype=float), float(r)) for name, c, r in spheres]
        self.P, self.O = int(n_planes), int(n_obstacles)
        self.base = (np.zeros(3), np.eye(3)) if base is None else (np.asarray(base[0], dtype=float), np.asarray(base[1], dtype=float).reshape(3, 3))
        self.links = [-1 if name is None else self.chain.poses(np.zeros(self.dof))[0][name][2] for name, _, _ in self.spheres]
        env, pairs = default_masks(self.links)
        self.env_mask = env if env_mask is None else int(env_mask)
        self.pair_mask = pairs if pair_mask is None else [int(x) for x in pair_mask]
        self.margins = tuple(float(m) for m in margins)

    # ---- kinematics through the independent chain
    def centres(self, q):
        """world centres [S][3] of one robot"""
        pb, Rb = self.base
        pos, _ = self.chain.poses(q)
        out = []
        for name, c, _ in self.spheres:
            if name is None:
                out.append(c.copy())
            else:
                R, p, _ = pos[name]
                out.append(pb + Rb @ (p + R @ c))
        return np.array(out)

    def point_jacobian(self, q, k):
        """d x_k / d q [3][dof] of one robot, world frame"""
        name, c, _ = self.spheres[k]
        if name is None:
            return np.zeros((3, self.dof))
        J, _, _ = self.chain.jacobian(q, name, c)
        return self.base[1] @ J[:3]

    # ---- the law
    def one(self, q, env, want_gradient=True):
        """q [dof], env [6 P + 4 O] of one robot -> dict with per category: distance, index, normal [3], gradient [dof], gap (the
        runner-up's distance minus the winner's, +inf with fewer than two candidates), norm (the centre distance that was
        normalised, +inf where none was); and centres [S][3], flags"""
        with np.errstate(invalid="ignore"):
            return self._one(q, env, want_gradient)

    def _one(self, q, env, want_gradient):
        S = len(self.spheres)
        x = self.centres(q)
        r = [s[2] for s in self.spheres]
        res = {}
        cands = {c: [] for c in CATEGORIES}  # (d, index) in loop order
        for p in range(self.P):
            p0, n = env[6 * p : 6 * p + 3], env[6 * p + 3 : 6 * p + 6]
            for k in range(S):
                if (self.env_mask >> k) & 1:
                    cands["plane"].append((float(n @ (x[k] - p0)) - r[k], 16 * p + k))
        for o in range(self.O):
            w = env[6 * self.P + 4 * o : 6 * self.P + 4 * o + 4]
            for k in range(S):
                if (self.env_mask >> k) & 1:
                    cands["obstacle"].append((float(np.linalg.norm(x[k] - w[:3])) - r[k] - w[3], 16 * o + k))
        for i in range(S):
            for j in range(i + 1, S):
                if (self.pair_mask[i] >> j) & 1:
                    cands["self"].append((float(np.linalg.norm(x[i] - x[j])) - r[i] - r[j], 16 * i + j))
        flags = 0
        for c, cat in enumerate(CATEGORIES):
            best, idx = np.inf, -1
            for d, i in cands[cat]:
                if d < best:  # false for a NaN
                    best, idx = d, i
            others = sorted(d for d, i in cands[cat] if i != idx and not np.isnan(d))
            u, g, norm = np.zeros(3), np.zeros(self.dof), np.inf
            if idx >= 0:
                a, k = idx >> 4, idx & 15
                if cat == "plane":
                    u = np.array(env[6 * a + 3 : 6 * a + 6], dtype=float)
                else:
                    e = x[k] - env[6 * self.P + 4 * a : 6 * self.P + 4 * a + 3] if cat == "obstacle" else x[a] - x[k]
                    norm = float(np.linalg.norm(e))
                    u = e / norm if norm > 0 else np.zeros(3)
                if want_gradient:
                    J = self.point_jacobian(q, k)
                    if cat == "self":
                        J = self.point_jacobian(q, a) - J
                    g = u @ J
            res[cat] = dict(distance=best, index=idx, normal=u, gradient=g, gap=(others[0] - best) if others and idx >= 0 else np.inf, norm=norm)
            if best < self.margins[c]:
                flags |= 1 << c
        if not np.all(np.isfinite(q)):
            flags = FLAG_NONFINITE
        res["centres"], res["flags"] = x, flags
        return res

    def evaluate(self, q, env=None, want_gradient=True):
        """q [dof][B], env [6 P + 4 O][B] -> arrays: distance [3][B], index [3][B], normal [9][B], gradient [3 dof][B], centres
        [3 S][B], flags [B] uint8, gap [3][B], norm [3][B], counts [5]"""
        n, B = q.shape
        S = len(self.spheres)
        out = dict(distance=np.empty((3, B)), index=np.empty((3, B)), normal=np.empty((9, B)), gradient=np.empty((3 * n, B)),
                   centres=np.empty((3 * S, B)), flags=np.zeros(B, dtype=np.uint8), gap=np.empty((3, B)), norm=np.empty((3, B)))
        env = np.zeros((0, B)) if env is None else env
        for b in range(B):
            r = self.one(q[:, b], env[:, b], want_gradient)
            for c, cat in enumerate(CATEGORIES):
                out["distance"][c, b], out["index"][c, b] = r[cat]["distance"], r[cat]["index"]
                out["normal"][3 * c : 3 * c + 3, b] = r[cat]["normal"]
                out["gradient"][n * c : n * c + n, b] = r[cat]["gradient"]
                out["gap"][c, b], out["norm"][c, b] = r[cat]["gap"], r[cat]["norm"]
            out["centres"][:, b] = r["centres"].reshape(-1)
            out["flags"][b] = r["flags"]
        f = out["flags"]
        out["counts"] = [int(((f >> k) & 1).sum()) for k in range(4)] + [int((f != 0).sum())]
        return out

    def output_rows(self, ev, blocks):
        """the [rows][B] output the product stores for `blocks` (names in flag order are taken in flag order)"""
        return np.concatenate([ev[k] for k in ("distance", "index", "normal", "gradient", "centres") if k in blocks], axis=0)


def product_spheres(pkg, links, spheres, base=None):
    """(link indices [S], centres [S][3] in the model's link frames, radii [S]) for the product's configuration. links: the
    UrdfLinks of pkg.model_from_urdf. A world sphere keeps its world centre."""
    idx, cen, rad = [], [], []
    for name, c, r in spheres:
        if name is None:
            idx.append(-1), cen.append(np.asarray(c, dtype=float))
        else:
            i, pos, R = pkg.resolve_link_frame(links, name)
            idx.append(i), cen.append(pos + R @ np.asarray(c, dtype=float))
        rad.append(float(r))
    return np.array(idx, dtype=np.int32), np.array(cen), np.array(rad)

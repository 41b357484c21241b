"""Per-robot payloads for the tests: 16 rigid bodies (robot b of a batch carries payload b % 16, so neighbouring lanes always
differ), each also rendered as URDF text — the robot's own URDF plus one <link> on a <joint type="fixed"> — which gives two
independent references for every robot: the C oracle on sai2b_model_from_urdf(text) (fixed bodies merged into their parent)
and tests/hp_reference.py (40 digits, a sum over the bodies of the text)."""
import numpy as np

import hp_fixture
import hp_reference as hp
import oracle_lib as ol
import sai2_primitives_perso_amd as pkg

P = 16


def payloads():
    """-> mass [16], com [3][16] (link frame), inertia [6][16] (about the COM, link axes: xx yy zz xy xz yz)"""
    rng = np.random.default_rng(20261016)
    m, c, I = np.zeros(P), np.zeros((3, P)), np.zeros((6, P))
    # 0: nothing attached
    m[1], c[:, 1] = 3.0, (0.2, 0.0, 0.05)  # the Panda's rated load as a point mass 0.2 m off the flange axis
    m[2], c[:, 2] = 1.5, (0.03, -0.04, 0.12)  # every product of inertia non-zero
    I[:, 2] = (0.020, 0.030, 0.025, 0.004, -0.006, 0.005)
    m[3], c[:, 3] = 0.05, (0.0, 0.01, 0.06)  # a light body
    I[:, 3] = (2e-5, 3e-5, 1e-5, 0.0, 0.0, 0.0)
    for k in range(4, P):
        m[k] = rng.uniform(0.1, 3.0)
        v = rng.normal(size=3)
        c[:, k] = v / np.linalg.norm(v) * rng.uniform(0.02, 0.15)
        A = rng.normal(size=(3, 3))
        S = A @ A.T
        S *= rng.uniform(0.005, 0.05) / np.abs(S).max()
        I[:, k] = (S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[0, 2], S[1, 2])
    return m, c, I


def rows(B, scale=None):
    """the rows of a batch of B robots: robot b carries payload b % 16 (scale: a factor on its mass and inertia)"""
    m, c, I = payloads()
    idx = np.arange(B) % P
    f = 1.0 if scale is None else scale
    return np.ascontiguousarray(m[idx] * f), np.ascontiguousarray(c[:, idx]), np.ascontiguousarray(I[:, idx] * f)


def link_name(text, link):
    """URDF name of moving link `link` (0-based: the child of the link-th non-fixed joint)"""
    return hp.Model(text).moving[link]["child"]


def urdf_with_payload(text, link, m, c, I):
    """the robot's URDF text with one more body on a fixed joint of moving link `link`; every number with 17 digits"""
    if m == 0 and not np.any(I):
        return text
    r = lambda x: repr(float(x))
    body = (f'<link name="payload"><inertial><origin xyz="{r(c[0])} {r(c[1])} {r(c[2])}" rpy="0 0 0"/><mass value="{r(m)}"/>'
            f'<inertia ixx="{r(I[0])}" iyy="{r(I[1])}" izz="{r(I[2])}" ixy="{r(I[3])}" ixz="{r(I[4])}" iyz="{r(I[5])}"/></inertial></link>\n'
            f'<joint name="payload_joint" type="fixed"><parent link="{link_name(text, link)}"/><child link="payload"/>'
            f'<origin xyz="0 0 0" rpy="0 0 0"/></joint>\n')
    at = text.rindex("</robot>")
    return text[:at] + body + text[at:]


def texts(robot="panda", link=None, scale=None):
    """the 16 URDF texts of a robot of tests/hp_fixture.py (default link: the last one)"""
    base = hp_fixture.urdf_text(robot)
    n = hp.Model(base).dof
    link = n - 1 if link is None else link
    m, c, I = payloads()
    f = 1.0 if scale is None else scale
    return [urdf_with_payload(base, link, m[k] * f, c[:, k], I[:, k] * f) for k in range(P)]


class PayloadOracles:
    """16 oracles, one per URDF text, each ticking the robots b with b % 16 == k; the calls of oracle_lib.Oracle that the
    tests use, on [rows][B] arrays of the whole batch"""

    def __init__(self, texts_, cfgs, B, threads=8):
        self.B = B
        self.idx = [np.arange(k, B, P) for k in range(P)]
        self.o = []
        for k in range(P):
            model, _ = pkg.model_from_urdf(texts_[k], is_file=False)
            self.o.append(ol.Oracle(model, cfgs, len(self.idx[k]), threads=threads) if len(self.idx[k]) else None)
        self.dof = int(model.dof)

    def _each(self):
        return [(o, i) for o, i in zip(self.o, self.idx) if o is not None]

    @staticmethod
    def _cut(a, i):
        return None if a is None else np.ascontiguousarray(np.asarray(a)[..., i])

    def call(self, name, *args, **kw):
        """o.<name>(...) on every oracle with every array argument cut to its robots; array results put together"""
        out = None
        for o, i in self._each():
            cut = lambda a: self._cut(a, i) if isinstance(a, np.ndarray) and a.ndim >= 1 and a.shape[-1] == self.B else a
            r = getattr(o, name)(*[cut(a) for a in args], **{k: cut(v) for k, v in kw.items()})
            if r is None:
                continue
            rs = r if isinstance(r, tuple) else (r,)
            if out is None:
                out = [np.empty(x.shape[:-1] + (self.B,), dtype=x.dtype) for x in rs]
            for dst, x in zip(out, rs):
                dst[..., i] = x
        if out is None:
            return None
        return tuple(out) if len(out) > 1 else out[0]

    def load_inputs(self, inp):
        def cut(v, i):
            if isinstance(v, dict):
                return {k: cut(x, i) for k, x in v.items()}
            return self._cut(v, i) if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[-1] == self.B else v

        for o, i in self._each():
            ol.load_inputs(o, cut(inp, i))

    def __getattr__(self, name):
        return lambda *a, **kw: self.call(name, *a, **kw)


# ---- the blending-region fixture tests/golden/hp_payload.npz (tests/golden/make_hp_payload_golden.py writes it) ----

HP_FIXTURE = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "hp_payload.npz")
# cells of tests/hp_fixture.py whose poses come from tests/singular_poses.py, 32 poses in all: a 3-row task (the in-lane
# singular branch of the 3-row SVD-free kernel), a 6-row one (the streamed branch of the 6-row kernel), and the 8-joint
# sliding-base Panda, whose 6-row task stands BEHIND a JointTask
HP_CELLS = {"six_r": 12, "six_r_mft6": 10, "sliding_base": 10}
# Where the MotionForceTask is the first task its singular values are those of J alone and a payload cannot change a robot's
# route. Behind another task they are those of J N_prec, and the dynamically consistent N_prec is built with M: there the
# payload may move a robot across the edge of the region (seen on sliding-base robots of the fixture).
HP_FIRST_TASK = ("six_r", "six_r_mft6")
HP_PAYLOADS = (1, 2)  # robot b carries payload HP_PAYLOADS[b % 2]: the 3 kg point mass and the body with products of inertia


def hp_texts(cell):
    """the URDF text per payload of HP_PAYLOADS, the payload on the cell's last link"""
    robot = hp_fixture.CELLS[cell]["robot"]
    t = texts(robot)
    return [t[k] for k in HP_PAYLOADS]


def hp_load(cell):
    z = np.load(HP_FIXTURE)
    return {k.split(".", 1)[1]: z[k] for k in z.files if k.split(".", 1)[0] == cell}


def model_rows(robot, link, m, c, I6):
    """payload rows given in the URDF link's frame -> (mass, com, inertia) in the model's link frame (z along the joint axis)"""
    text = hp_fixture.urdf_text(robot)
    _, links = pkg.model_from_urdf(text, is_file=False)
    idx, pos, R = pkg.resolve_link_frame(links, link_name(text, link))
    assert idx == link
    I = np.einsum("ij,jkb,lk->ilb", R, np.stack([I6[[0, 3, 4]], I6[[3, 1, 5]], I6[[4, 5, 2]]]), R)
    return m, np.ascontiguousarray(pos[:, None] + R @ c), np.ascontiguousarray(np.stack([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]))


def hp_rows(cell, B):
    m, c, I = payloads()
    idx = np.array(HP_PAYLOADS)[np.arange(B) % len(HP_PAYLOADS)]
    robot = hp_fixture.CELLS[cell]["robot"]
    n = hp.Model(hp_fixture.urdf_text(robot)).dof
    return n - 1, model_rows(robot, n - 1, np.ascontiguousarray(m[idx]), np.ascontiguousarray(c[:, idx]), np.ascontiguousarray(I[:, idx]))


def hp_make(cell, d, mk_jt, mk_mft, make_ctrl, model=None):
    """a controller for the cell's robots (hierarchy and options of tests/hp_fixture.py), goals of the fixture loaded"""
    mdl, links = hp_fixture.product_model(hp_fixture.CELLS[cell]["robot"])
    cfgs = hp_fixture.product_configs(cell, mk_jt, mk_mft, links)
    ctrl = make_ctrl(mdl if model is None else model, cfgs, d["dq"].shape[1])
    for t, k in enumerate(hp_fixture.kinds(cell)):
        if k == "mft":
            ctrl.set_mft_goals(t, *[np.ascontiguousarray(d[f"mft{t}_{x}"]) for x in ("pos", "rot", "v", "w", "a", "alpha")])
        else:
            ctrl.set_jt_goals(t, *[np.ascontiguousarray(d[f"jt{t}_{x}"]) for x in ("q", "dq", "ddq")])
    return ctrl

"""The premise of tests/test_gpu_robot_routes.py, checked without a GPU: the poses of tests/singular_poses.py land in the
singularity band they were drawn for, as the CPU oracle classifies them (get_mft_singularity: the split index and the
blending factor of the SingularityHandler)."""
import numpy as np
import pytest

import oracle_lib as ol
import singular_poses as sp
import robots
import sai2_primitives_perso_amd as pkg

HIER = {"planar_4r": ("planar_4r", False), "six_r": ("six_r", False), "six_r_mft6": ("six_r", True), "sliding_base": ("sliding_base", False)}


def _oracle(name, q):
    """the oracle with the hierarchy of test_gpu_robots._setup for this task, at the poses q"""
    robot, mft6 = HIER[name]
    m, links = pkg.model_from_urdf(robots.TEXT[robot](), is_file=False)
    n, B = m.dof, q.shape[1]
    if robot == "sliding_base":
        link, fpos, frot = pkg.resolve_link_frame(links, "end-effector", (0.0, 0.0, 0.07))
        sel = np.zeros((2, n))
        sel[0, 0] = sel[1, 7] = 1
        cfg = [ol.joint_task("partial_joint_task", sel, robot_dof=n), ol.motion_force_task("motion_force_task", link, fpos, frot, robot_dof=n),
               ol.joint_task("joint_task", None, robot_dof=n)]
        t = 1
    else:
        pt = {"planar_4r": ("link4", (0.5, 0.0, 0.0)), "six_r": ("link6", (0.05, 0.0, 0.02))}[robot]
        link, fpos, frot = pkg.resolve_link_frame(links, *pt)
        partial = None if mft6 else ((np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[0, 0, 1.0]])) if robot == "planar_4r"
                                     else (np.eye(3), np.zeros((0, 3))))
        cfg = [ol.motion_force_task("motion_force_task", link, fpos, frot, partial, robot_dof=n)]
        t = 0
    o = ol.Oracle(m, cfg, B, threads=8)
    o.set_state(np.ascontiguousarray(q), np.zeros((n, B)))
    o.reinitialize()
    o.tick()
    return o, t


@pytest.mark.parametrize("name", list(sp.TASKS))
def test_every_band_is_populated_as_intended(name):
    bands = sp.TASKS[name]["bands"]
    q, band = sp.mixed(name, 16 * len(bands))
    o, t = _oracle(name, q)
    _, alpha, ro = o.get_mft_singularity(t)
    rank = o.tasks[t].pos_range + o.tasks[t].ori_range
    assert rank == len(sp.TASKS[name]["rows"])
    want = {"regular": (ro == rank), "blending": (ro == rank - 1) & (alpha > 0) & (alpha < 1),
            "inside": (ro == rank - 1) & (alpha == 0), "two": (ro <= rank - 2)}
    for k, b in enumerate(sp.BANDS):
        sel = band == k
        assert (b in bands) == bool(sel.any()), b
        assert want[b][sel].all(), (b, ro[sel], alpha[sel])

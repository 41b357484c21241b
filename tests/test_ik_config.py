"""Host-only checks of the inverse-kinematics configuration (include/sai2b.h "inverse kinematics"), no GPU: the defaults, every
rejection of sai2b_validate_ik (those that hang on the model's limits included), sai2b_ik_input_rows, the ctypes mirror's size, and
the argument checks of the context calls that need no context."""
import ctypes as C

import numpy as np
import pytest

import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi


def _model():
    return pkg.panda_model()


def _validate(cfg, dof=7, lower=None, upper=None):
    lib = _abi.load_library()
    msg = C.create_string_buffer(256)
    lo = None if lower is None else C.c_void_p(np.ascontiguousarray(lower, dtype=np.float64).ctypes.data)
    hi = None if upper is None else C.c_void_p(np.ascontiguousarray(upper, dtype=np.float64).ctypes.data)
    return lib.sai2b_validate_ik(C.byref(cfg), dof, lo, hi, msg, 256), msg.value.decode()


def test_the_ctypes_mirror_has_the_library_size():
    lib = _abi.load_library()
    assert lib.sai2b_sizeof_ik_config() == C.sizeof(_abi.IkConfig) == 168


def test_the_defaults():
    lib = _abi.load_library()
    cfg = _abi.IkConfig()
    assert lib.sai2b_default_ik(C.byref(cfg)) == 0
    assert (cfg.task, cfg.axes, cfg.max_iterations, cfg.restarts, cfg.use_limits, cfg.view, cfg.goal_source, cfg.seed_source) == (0, 63, 40, 0, 1, 0, 0, 0)
    assert (cfg.rot_length, cfg.tol_pos, cfg.tol_rot, cfg.mu0, cfg.mu_min, cfg.mu_max, cfg.mu_down, cfg.mu_up) == (0.25, 1e-6, 1e-6, 1e-2, 1e-9, 1e3, 0.25, 8.0)
    assert (cfg.step_max, cfg.limit_margin, cfg.rest_weight, cfg.seed, cfg.first_robot, cfg.draw_id) == (0.5, 0.0, 0.0, 0, 0, 0)
    assert _validate(cfg) == (0, "")
    assert lib.sai2b_default_ik(None) == _abi.INVALID_ARGUMENT
    same = pkg.ik_config(_model())
    assert bytes(same) == bytes(cfg)


def _set(field, value):
    return lambda cfg: setattr(cfg, field, value)


NAN, INF = float("nan"), float("inf")
REJECTED = [
    ("task", _set("task", -1)), ("task", _set("task", 4)),
    ("axes", _set("axes", 0)), ("axes", _set("axes", 64)), ("axes", _set("axes", -1)),
    ("rot_length", _set("rot_length", 0.0)), ("rot_length", _set("rot_length", -1.0)), ("rot_length", _set("rot_length", NAN)), ("rot_length", _set("rot_length", INF)),
    ("max_iterations", _set("max_iterations", 0)), ("max_iterations", _set("max_iterations", 201)),
    ("restarts", _set("restarts", -1)), ("restarts", _set("restarts", 17)),
    ("tol_pos", _set("tol_pos", -1e-9)), ("tol_pos", _set("tol_rot", NAN)), ("tol_pos", _set("tol_pos", INF)),
    ("damping", _set("mu_min", 0.0)), ("damping", _set("mu0", 1e-10)), ("damping", _set("mu0", 1e4)), ("damping", _set("mu_max", INF)), ("damping", _set("mu0", NAN)),
    ("mu_down", _set("mu_down", 0.0)), ("mu_down", _set("mu_down", 1.0)), ("mu_down", _set("mu_down", NAN)),
    ("mu_up", _set("mu_up", 1.0)), ("mu_up", _set("mu_up", INF)), ("mu_up", _set("mu_up", NAN)),
    ("step_max", _set("step_max", 0.0)), ("step_max", _set("step_max", NAN)), ("step_max", _set("step_max", INF)),
    ("use_limits", _set("use_limits", 2)),
    ("limit_margin", _set("limit_margin", -0.01)), ("limit_margin", _set("limit_margin", NAN)),
    ("rest_weight", _set("rest_weight", -1.0)), ("rest_weight", _set("rest_weight", INF)),
    ("view", _set("view", 2)), ("view", _set("view", -1)),
    ("goal_source", _set("goal_source", 2)), ("seed_source", _set("seed_source", -1)),
]


@pytest.mark.parametrize("word, change", REJECTED, ids=[f"{k}-{w}" for k, (w, _) in enumerate(REJECTED)])
def test_the_validator_rejects(word, change):
    cfg = pkg.ik_config(_model())
    change(cfg)
    rc, msg = _validate(cfg)
    assert rc == _abi.INVALID_ARGUMENT and word in msg, msg
    lib = _abi.load_library()
    assert lib.sai2b_ik_input_rows(C.byref(cfg), 7, None, None) == _abi.INVALID_ARGUMENT
    assert word in lib.sai2b_last_error(None).decode()


def test_what_hangs_on_the_limits():
    m = _model()
    lo, hi = np.array(m.q_lower[:7]), np.array(m.q_upper[:7])
    cfg = pkg.ik_config(m, restarts=3, limit_margin=0.01)
    assert _validate(cfg, 7, lo, hi) == (0, "") and _validate(cfg) == (0, "")
    # restarts without limits in use; with a limit that is not finite; a margin that leaves no interval; one array alone
    cfg.use_limits = 0
    assert "restarts need use_limits" in _validate(cfg, 7, lo, hi)[1] and "restarts need use_limits" in _validate(cfg)[1]
    cfg.use_limits = 1
    for bad in (INF, -INF):
        up = hi.copy()
        up[3] = bad if bad > 0 else up[3]
        dn = lo.copy()
        dn[2] = bad if bad < 0 else dn[2]
        assert "finite limits" in _validate(cfg, 7, dn, up)[1]
        cfg.restarts = 0
        assert _validate(cfg, 7, dn, up) == (0, "")  # an unbounded joint is fine without restarts
        cfg.restarts = 3
    up = hi.copy()
    up[5] = NAN
    assert "interval" in _validate(cfg, 7, lo, up)[1]
    cfg.limit_margin = 3.0
    assert "interval" in _validate(cfg, 7, lo, hi)[1]
    cfg.limit_margin = 0.0
    assert "together" in _validate(cfg, 7, lo, None)[1]
    with pytest.raises(ValueError, match="interval"):
        pkg.ik_config(m, limit_margin=3.0)
    with pytest.raises(ValueError, match="axes are"):
        pkg.ik_config(m, axes=("x", "w"))
    assert pkg.ik_config(m, axes=("x", "y", "wz")).axes == 0b100011


def test_the_validator_accepts_the_edges_and_needs_a_known_robot_size():
    m = _model()
    cfg = pkg.ik_config(m, task=3, axes=1, max_iterations=200, restarts=16, tol_pos=0.0, tol_rot=0.0, mu0=1e-9, mu_min=1e-9, mu_max=1e-9, mu_down=0.999,
                        mu_up=1.001, rest_weight=2.0, view="measured", goal_source="task", seed_source="state", seed=2**64 - 1, first_robot=2**32 - 1,
                        draw_id=2**32 - 1)
    assert _validate(cfg) == (0, "")
    assert _validate(cfg, 5)[0] != 0 and _validate(cfg, 0)[0] != 0 and _validate(cfg, 4)[0] == 0
    lib = _abi.load_library()
    assert lib.sai2b_validate_ik(None, 7, None, None, None, 0) == _abi.INVALID_ARGUMENT


def test_the_input_rows():
    lib = _abi.load_library()
    g, s = C.c_int(), C.c_int()
    for dof, model in ((7, _model()),):
        for goal_source, seed_source, nu, want in (("rows", "rows", 0.0, (12, dof)), ("rows", "state", 0.5, (12 + dof, 0)), ("task", "rows", 0.0, (0, dof)),
                                                   ("task", "state", 0.5, (dof, 0))):
            cfg = pkg.ik_config(model, goal_source=goal_source, seed_source=seed_source, rest_weight=nu)
            assert lib.sai2b_ik_input_rows(C.byref(cfg), dof, C.byref(g), C.byref(s)) == 0 and (g.value, s.value) == want
    assert lib.sai2b_ik_input_rows(C.byref(cfg), 6, C.byref(g), C.byref(s)) == 0 and (g.value, s.value) == (6, 0)  # the 6-joint build's answer
    assert lib.sai2b_ik_input_rows(C.byref(cfg), 5, C.byref(g), C.byref(s)) != 0


def test_context_calls_without_a_context():
    lib = _abi.load_library()
    cfg = pkg.ik_config(_model())
    counts = (C.c_int * 4)()
    assert lib.sai2b_set_ik(None, C.byref(cfg)) == _abi.INVALID_ARGUMENT and "null ctx" in lib.sai2b_last_error(None).decode()
    assert lib.sai2b_clear_ik(None) == _abi.INVALID_ARGUMENT and lib.sai2b_get_ik(None, C.byref(cfg)) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_solve_ik(None, None, None, None, None, None, None, 0) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_get_ik_counts(None, counts) == _abi.INVALID_ARGUMENT

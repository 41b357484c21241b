"""Host-only checks of the collision configuration (include/sai2b.h "collision proximity"), no GPU: every rejection of
sai2b_validate_collision, the layout arithmetic of sai2b_collision_config_layout for every block subset at 4 and 8 joints, the
default masks of sai2b_default_collision against tests/collision_reference.default_masks, the ctypes mirror's size, and the
argument checks of sai2b_end_episodes that need no context."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sai2_primitives_perso_amd as pkg
from collision_reference import default_masks
from sai2_primitives_perso_amd import _abi

LINKS = [-1, 0, 1, 2, 3, 3]
CENTRES = np.arange(18, dtype=float).reshape(6, 3) * 0.01
RADII = [0.05, 0.04, 0.03, 0.02, 0.01, 0.0]


def _good(dof=4, **kw):
    return pkg.collision_config(dof, LINKS, CENTRES, RADII, **kw)


def _validate(cfg, dof=4):
    lib = _abi.load_library()
    msg = C.create_string_buffer(256)
    return lib.sai2b_validate_collision(C.byref(cfg), dof, msg, 256), msg.value.decode()


def test_the_ctypes_mirror_has_the_library_size():
    lib = _abi.load_library()
    assert lib.sai2b_sizeof_collision_config() == C.sizeof(_abi.CollisionConfig) == 720


def test_the_defaults():
    cfg = _good(n_planes=2, n_obstacles=4)
    assert (cfg.n_spheres, cfg.blocks, cfg.view) == (6, _abi.COL_DISTANCE, 0) and (cfg.margin_plane, cfg.margin_obstacle, cfg.margin_self) == (0, 0, 0)
    assert list(cfg.link[:6]) == LINKS and np.array_equal(np.array([list(c) for c in cfg.centre[:6]]), CENTRES) and list(cfg.radius[:6]) == RADII
    env, pairs = default_masks(LINKS)
    assert cfg.env_mask == env == 0b111110 and list(cfg.pair_mask) == pairs
    assert _validate(cfg) == (0, "")
    # links 3 and 3, 2 and 3: not tested; -1 and 1: tested (-1 counts as a link)
    assert not (cfg.pair_mask[4] >> 5) & 1 and not (cfg.pair_mask[3] >> 4) & 1 and (cfg.pair_mask[0] >> 2) & 1 and not (cfg.pair_mask[0] >> 1) & 1
    lib = _abi.load_library()
    raw = _abi.CollisionConfig()
    links, rad = np.array(LINKS, dtype=np.int32), np.array(RADII)
    for n in (0, 17):
        assert lib.sai2b_default_collision(C.byref(raw), n, links.ctypes.data, CENTRES.ctypes.data, rad.ctypes.data) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_default_collision(C.byref(raw), 6, None, CENTRES.ctypes.data, rad.ctypes.data) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_default_collision(None, 6, links.ctypes.data, CENTRES.ctypes.data, rad.ctypes.data) == _abi.INVALID_ARGUMENT


def _set(field, value, index=None):
    def change(cfg):
        if index is None:
            setattr(cfg, field, value)
        elif isinstance(index, tuple):
            getattr(cfg, field)[index[0]][index[1]] = value
        else:
            getattr(cfg, field)[index] = value

    return change


REJECTED = [
    ("n_spheres", _set("n_spheres", 0)), ("n_spheres", _set("n_spheres", 17)), ("n_planes", _set("n_planes", -1)), ("n_planes", _set("n_planes", 3)),
    ("n_obstacles", _set("n_obstacles", -1)), ("n_obstacles", _set("n_obstacles", 5)),
    ("link", _set("link", -2, 1)), ("link", _set("link", 4, 5)),
    ("centre", _set("centre", float("nan"), (2, 1))), ("centre", _set("centre", float("inf"), (0, 0))),
    ("radius", _set("radius", -1e-9, 3)), ("radius", _set("radius", float("nan"), 0)), ("radius", _set("radius", float("inf"), 5)),
    ("env_mask", _set("env_mask", 1 << 6)), ("pair_mask", _set("pair_mask", 1 << 6, 0)), ("pair_mask", _set("pair_mask", 1, 7)),
    ("i < j", _set("pair_mask", 0b100, 2)), ("i < j", _set("pair_mask", 0b001000 | 0b000001, 3)),
    ("blocks", _set("blocks", 32)), ("blocks", _set("blocks", -1)),
    ("margin", _set("margin_plane", float("nan"))), ("margin", _set("margin_obstacle", float("inf"))), ("margin", _set("margin_self", float("-inf"))),
    ("view", _set("view", 2)), ("view", _set("view", -1)),
]


@pytest.mark.parametrize("word, change", REJECTED, ids=[f"{k}-{w}" for k, (w, _) in enumerate(REJECTED)])
def test_the_validator_rejects(word, change):
    cfg = _good(n_planes=1, n_obstacles=1)
    change(cfg)
    rc, msg = _validate(cfg)
    assert rc == _abi.INVALID_ARGUMENT and word in msg, msg
    lib = _abi.load_library()
    assert lib.sai2b_collision_config_layout(C.byref(cfg), 4, _abi.COL_DISTANCE, -1, None, None, None, None) == _abi.INVALID_ARGUMENT


def test_the_validator_accepts_the_edges_and_needs_a_known_robot_size():
    cfg = _good(8, n_planes=2, n_obstacles=4, blocks=tuple(_abi.COL_BLOCKS), view="measured", pairs="all", margin_self=-0.5)
    cfg.link[5] = 7
    assert _validate(cfg, 8) == (0, "")
    assert _validate(cfg, 4)[0] == _abi.INVALID_ARGUMENT  # link 7 on a 4-joint robot
    assert _validate(_good(), 5)[0] != 0 and _validate(_good(), 0)[0] != 0
    lib = _abi.load_library()
    assert lib.sai2b_validate_collision(None, 4, None, 0) == _abi.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        pkg.collision_config(4, LINKS, CENTRES[:5], RADII)
    with pytest.raises(ValueError, match="block"):
        _good(blocks=("distance", "depth"))
    with pytest.raises(ValueError):
        _good(pairs=[(2, 1)])


@pytest.mark.parametrize("dof", [4, 8])
def test_the_layout_of_every_block_subset(dof):
    lib = _abi.load_library()
    names = list(_abi.COL_BLOCKS)
    S = len(LINKS)
    sizes = dict(distance=3, index=3, normal=9, gradient=3 * dof, centres=3 * S)
    first, n, total, env = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    for k in range(len(names) + 1):
        for subset in itertools.combinations(names, k):
            cfg = _good(dof, n_planes=1, n_obstacles=3, blocks=subset)
            row = 0
            for name in names:
                assert lib.sai2b_collision_config_layout(C.byref(cfg), dof, _abi.COL_BLOCKS[name], -1, C.byref(first), C.byref(n), C.byref(total), C.byref(env)) == 0
                assert total.value == sum(sizes[b] for b in subset) and env.value == 6 + 12
                if name not in subset:
                    assert (first.value, n.value) == (-1, 0)
                    continue
                assert (first.value, n.value) == (row, sizes[name]), (subset, name)
                for cat in range(3):
                    rc = lib.sai2b_collision_config_layout(C.byref(cfg), dof, _abi.COL_BLOCKS[name], cat, C.byref(first), C.byref(n), None, None)
                    if name == "centres":
                        assert rc == _abi.INVALID_ARGUMENT
                    else:
                        per = sizes[name] // 3
                        assert rc == 0 and (first.value, n.value) == (row + per * cat, per)
                row += sizes[name]
    cfg = _good(dof)
    for block in (0, 3, 32, -1):
        assert lib.sai2b_collision_config_layout(C.byref(cfg), dof, block, -1, None, None, None, None) == _abi.INVALID_ARGUMENT
    for cat in (-2, 3):
        assert lib.sai2b_collision_config_layout(C.byref(cfg), dof, _abi.COL_DISTANCE, cat, None, None, None, None) == _abi.INVALID_ARGUMENT
    assert lib.sai2b_collision_config_layout(C.byref(cfg), 5, _abi.COL_DISTANCE, -1, None, None, None, None) != 0


def test_end_episodes_rejects_without_a_context():
    lib = _abi.load_library()
    done, extra = np.zeros(4, dtype=np.uint8), np.ones(4, dtype=np.uint8)
    for bit in (0, 1, 2, 4, 8, 16, 32, 63, 65, 96, 127, 129, 192, 256, -64):
        assert lib.sai2b_end_episodes(None, done.ctypes.data, extra.ctypes.data, bit, 0) == _abi.INVALID_ARGUMENT
        assert "bit must be 64 or 128" in lib.sai2b_last_error(None).decode()
    for bit in (64, 128):
        assert lib.sai2b_end_episodes(None, None, extra.ctypes.data, bit, 0) == _abi.INVALID_ARGUMENT
        assert "required" in lib.sai2b_last_error(None).decode()
        assert lib.sai2b_end_episodes(None, done.ctypes.data, None, bit, 0) == _abi.INVALID_ARGUMENT
        assert lib.sai2b_end_episodes(None, done.ctypes.data, extra.ctypes.data, bit, 0) == _abi.INVALID_ARGUMENT
        assert "null ctx" in lib.sai2b_last_error(None).decode()
    assert not done.any() and extra.all() and _abi.DONE_COLLISION == 64 and _abi.DONE_COLLISION not in _abi.DONE_BITS.values()
    count = C.c_int(7)
    assert lib.sai2b_get_end_episode_count(None, C.byref(count)) == _abi.INVALID_ARGUMENT
    for fn in ("sai2b_clear_collision", "sai2b_collision_rows"):
        assert getattr(lib, fn)(None) in (_abi.INVALID_ARGUMENT, -1)
    assert lib.sai2b_collision_query(None, None, None, 0) == _abi.INVALID_ARGUMENT and lib.sai2b_set_collision(None, None, None, 0) == _abi.INVALID_ARGUMENT

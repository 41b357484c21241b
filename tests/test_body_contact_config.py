"""The configuration of the whole-arm contact (include/sai2b.h "whole-arm contact") on the host: no GPU, no context.

The ctypes mirror has the library's size; the defaults; every rejection of the validator; the entry points that take a context
refuse a NULL one as a bad argument (the setter without a collision configuration needs a context and is in
tests/test_gpu_body_contact.py); the status layout the header, the law's header and the Python mirror state is one layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
INVALID = 1


def _lib():
    return _abi.load_library()


def _validate(cfg, dof=7):
    msg = C.create_string_buffer(256)
    rc = _lib().sai2b_validate_body_contact(C.byref(cfg) if cfg is not None else None, dof, msg, 256)
    return rc, msg.value.decode()


def test_the_ctypes_mirror_has_the_library_size():
    assert _lib().sai2b_sizeof_body_contact_config() == C.sizeof(_abi.BodyContactConfig) == 48


def test_the_defaults():
    cfg = _abi.BodyContactConfig()
    cfg.categories, cfg.v_eps, cfg.reserved0 = 99, -1.0, 5
    assert _lib().sai2b_default_body_contact(C.byref(cfg)) == 0
    assert cfg.categories == 7 and cfg.v_eps == 1e-3 and cfg.reserved0 == 0 and list(cfg.reserved) == [0] * 8
    assert _lib().sai2b_default_body_contact(None) != 0
    for dof in (4, 6, 7, 8):
        assert _validate(cfg, dof) == (0, "")
    c2 = pkg.body_contact_config(7, categories=("plane", "self"), v_eps=2e-3)
    assert c2.categories == 5 and c2.v_eps == 2e-3
    assert pkg.body_contact_config(6, categories="obstacle").categories == 2 and pkg.body_contact_config(4, categories=3).categories == 3


@pytest.mark.parametrize("word, change", [
    ("selects nothing", dict(categories=0)),
    ("unknown bits", dict(categories=8)),
    ("unknown bits", dict(categories=-1)),
    ("v_eps", dict(v_eps=0.0)),
    ("v_eps", dict(v_eps=-1e-3)),
    ("v_eps", dict(v_eps=float("nan"))),
    ("v_eps", dict(v_eps=float("inf"))),
])
def test_the_validator_rejects(word, change):
    cfg = pkg.body_contact_config(7)
    for k, v in change.items():
        setattr(cfg, k, v)
    rc, msg = _validate(cfg)
    assert rc != 0 and word in msg, (rc, msg)
    with pytest.raises(ValueError, match=word):
        pkg.body_contact_config(7, categories=change.get("categories", 7), v_eps=change.get("v_eps", 1e-3))


def test_the_validator_needs_a_config_and_a_known_robot_size():
    rc, msg = _validate(None)
    assert rc != 0 and "null config" in msg
    cfg = pkg.body_contact_config(7)
    for dof in (0, 3, 5, 9):
        assert _validate(cfg, dof)[0] != 0
    with pytest.raises(ValueError, match="category"):
        pkg.body_contact_config(7, categories=("floor",))


def test_the_entry_points_refuse_a_null_context():
    lib = _lib()
    cfg = pkg.body_contact_config(7)
    rows = np.zeros((3, 4))
    counts = (C.c_int * 4)()
    assert lib.sai2b_set_body_contact(None, C.byref(cfg), C.c_void_p(rows.ctypes.data), 0) == INVALID
    assert b"null ctx" in lib.sai2b_last_error(None)
    assert lib.sai2b_clear_body_contact(None) == INVALID
    assert lib.sai2b_get_body_contact(None, C.byref(cfg), None) == INVALID
    assert lib.sai2b_get_body_contact_state(None, None, counts) == INVALID


def test_the_status_layout_is_one_layout():
    """rows 0-2 depth, 3-5 witness, 6-8 sum of f_n, 9.. tb; four counts; buffers 25 and 26: the public header, the law's header and
    the Python mirror"""
    law = open(os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc", "sai2b_body_contact_law.h")).read()
    m = re.search(r"BC_DEPTH = (\d+), BC_INDEX = (\d+), BC_FSUM = (\d+), BC_TORQUE = (\d+)", law)
    assert m and [int(x) for x in m.groups()] == [0, 3, 6, 9]
    assert re.search(r"BC_ROWS = 3;", law) and re.search(r"BC_COUNTS = 4;", law)
    pub = open(os.path.join(ROOT, "include", "sai2b.h")).read()
    assert re.search(r"SAI2B_BUF_BODY_CONTACT = 25,", pub) and re.search(r"SAI2B_BUF_BODY_CONTACT_STATUS = 26\b", pub)
    assert "[9 + dof][B]" in pub and "int counts[4]" in pub
    assert (_abi.BUF_BODY_CONTACT, _abi.BUF_BODY_CONTACT_STATUS) == (25, 26)
    assert _abi.BODY_CONTACT_COUNTS == ("plane", "obstacle", "self", "any")
    assert [1 << _abi.COL_CATEGORIES.index(c) for c in ("plane", "obstacle", "self")] == [1, 2, 4]

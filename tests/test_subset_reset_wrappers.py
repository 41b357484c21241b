"""CPU tests of the Python side of the masked re-initialisation and the episode reset: sharding.reset_robots /
reinitialize_robots hand each rank the mask entries and state columns of its shard, and Controller's wrappers reject a
mask or rows of the wrong shape or dtype before any library call (the library object here fails the test if it is
touched)."""
import numpy as np
import pytest

from sai2_primitives_perso_amd import controller, sharding


class _Recorder:
    def __init__(self):
        self.calls = []

    def reset_robots(self, mask, q=None, dq=None):
        self.calls.append(("reset", mask, q, dq))

    def reinitialize_robots(self, mask, task=-1):
        self.calls.append(("reinit", mask, task))


def test_shard_helpers_slice_mask_and_rows_by_the_shard_bounds():
    B, world = 11, 3  # shards of 4, 4, 3
    mask = (np.arange(B) % 3 == 0)
    q, dq = np.arange(7 * B, dtype=np.float64).reshape(7, B), -np.arange(7 * B, dtype=np.float64).reshape(7, B)
    seen = np.zeros(B, dtype=bool)
    for rank in range(world):
        lo, hi = sharding.shard_bounds(B, world, rank)
        rec = _Recorder()
        sharding.reset_robots(rec, world, rank, mask, q, dq)
        sharding.reset_robots(rec, world, rank, mask.astype(np.uint8))
        sharding.reinitialize_robots(rec, world, rank, mask, task=1)
        (_, m, qs, dqs), (_, m8, q_none, dq_none), (_, mr, task) = rec.calls
        assert m.shape == (hi - lo,) and m.dtype == np.bool_ and np.array_equal(m, mask[lo:hi])
        assert m8.dtype == np.uint8 and np.array_equal(m8, mask[lo:hi]) and q_none is None and dq_none is None
        assert np.array_equal(qs, q[:, lo:hi]) and np.array_equal(dqs, dq[:, lo:hi]) and qs.flags.c_contiguous
        assert np.array_equal(mr, mask[lo:hi]) and task == 1
        seen[lo:hi] = True
    assert seen.all()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


def _bare(B=6, dof=7, n_tasks=2):
    c = object.__new__(controller.Controller)
    c.lib, c.h, c.B, c.dof, c.tasks, c._caller_stream = _NoLibrary(), None, B, dof, [None] * n_tasks, 0
    return c


@pytest.mark.parametrize("mask", [np.ones(5, dtype=bool), np.ones(7, dtype=np.uint8), np.ones((1, 6), dtype=bool), np.ones(6), np.ones(6, dtype=np.int32),
                                  np.ones(6, dtype=np.int8), None, [1, 0, 1, 0, 1, 0]])
def test_wrappers_reject_a_bad_mask_before_the_library(mask):
    c = _bare()
    with pytest.raises(ValueError):
        c.reset_robots(mask)
    with pytest.raises(ValueError):
        c.reinitialize_robots(mask)
    with pytest.raises(ValueError):
        c.reinitialize_robots(mask, task=0)


def test_wrappers_reject_bad_rows_and_tasks_before_the_library():
    c = _bare()
    ok = np.ones(6, dtype=bool)
    for q, dq in ((np.zeros((7, 5)), None), (None, np.zeros((6, 6))), (np.zeros(42), None)):
        with pytest.raises(ValueError):
            c.reset_robots(ok, q, dq)
    for task in (2, -2, 7):
        with pytest.raises(ValueError):
            c.reinitialize_robots(ok, task=task)
    # accepted arguments do reach the library
    for call in (lambda: c.reset_robots(ok, np.zeros((7, 6)), np.zeros((7, 6))), lambda: c.reinitialize_robots(ok.astype(np.uint8), task=1)):
        with pytest.raises(AssertionError, match="library call"):
            call()

"""Multi-GPU bookkeeping: robots are independent, so a node run shards the batch —
one process per GPU, contiguous shards generated per rank, NO collective on the data path. The only
communication is the timing protocol of bench.py: a barrier and a MAX-reduction of two scalars.
Both go over "gloo" by default, on GPUs too: with no exchange step on the path there is nothing for an RCCL
communicator to carry, and the timing protocol should not depend on one coming up ("nccl" = RCCL can be asked for)."""
import os

import torch
import torch.distributed as dist


def env_rank():
    """(rank, local_rank, world) from the torch.distributed.run environment"""
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def init(backend, local_rank=0):
    rank, _, world = env_rank()
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        kw = {}
        if backend == "nccl":
            kw["device_id"] = torch.device("cuda", local_rank)
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    return rank, world


def barrier():
    if dist.is_initialized():
        dist.barrier()


def max_over_ranks(values, device="cpu"):
    """element-wise MAX of a list of floats over all ranks (identity when not distributed)"""
    if not dist.is_initialized():
        return list(values)
    t = torch.tensor(list(values), dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return [float(x) for x in t]


def shard_bounds(global_batch, world, rank):
    """contiguous slice [lo, hi) of a global batch owned by `rank` (remainder spread over low ranks)"""
    base, rem = divmod(global_batch, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_rows(a, world, rank):
    """the columns [lo, hi) of a [rows][global_batch] (or [global_batch]) array or tensor that `rank` owns; None stays None"""
    if a is None:
        return None
    lo, hi = shard_bounds(a.shape[-1], world, rank)
    part = a[..., lo:hi]
    return part.contiguous() if hasattr(part, "contiguous") else part.copy()


def set_link_payload(ctrl, world, rank, link, mass, com=None, inertia=None, target="both"):
    """Controller.set_link_payload on this rank's shard of per-robot payload rows given for the whole batch"""
    ctrl.set_link_payload(link, *[shard_rows(a, world, rank) for a in (mass, com, inertia)], target=target)


def set_external_wrench(ctrl, world, rank, link, force, moment=None, steps=None, **kwargs):
    """Controller.set_external_wrench on this rank's shard of per-robot force / moment rows [3][global_batch] and steps
    [global_batch] given for the whole batch (a [3] force or moment, or a scalar steps, is batch-uniform and passes as it is)"""

    def part(a, ndim):
        return shard_rows(a, world, rank) if a is not None and getattr(a, "ndim", 0) == ndim else a

    ctrl.set_external_wrench(link, part(force, 2), part(moment, 2), part(steps, 1), **kwargs)


def set_hardware(ctrl, world, rank, global_batch, actuator_rows=None, sensor_rows=None, **kwargs):
    """Controller.set_hardware on this rank's shard of the per-robot rows [..][global_batch] given for the whole batch, with
    first_robot set to the shard's first global index: every robot draws the noise it draws in the one-context run"""
    lo, _ = shard_bounds(global_batch, world, rank)
    ctrl.set_hardware(shard_rows(actuator_rows, world, rank), shard_rows(sensor_rows, world, rank), first_robot=lo, **kwargs)


def set_joint_sensor(ctrl, world, rank, global_batch, rows=None, **kwargs):
    """Controller.set_joint_sensor on this rank's shard of the per-robot rows [1 + 5 dof][global_batch] given for the whole
    batch, with first_robot set to the shard's first global index: every robot draws the noise it draws in the one-context run"""
    lo, _ = shard_bounds(global_batch, world, rank)
    ctrl.set_joint_sensor(shard_rows(rows, world, rank), first_robot=lo, **kwargs)


def set_collision(ctrl, world, rank, global_batch, cfg, rows=None):
    """Controller.set_collision on this rank's shard of the per-robot environment rows [6 P + 4 O][global_batch] given for the
    whole batch; the configuration is batch-uniform and goes to every shard as it is"""
    ctrl.set_collision(cfg, shard_rows(rows, world, rank))


def set_ik(ctrl, world, rank, global_batch, **kwargs):
    """Controller.set_ik with first_robot set to the shard's first global index: every robot draws the restart seeds it draws
    in the one-context run. The rows of solve_ik are sharded with shard_rows."""
    lo, _ = shard_bounds(global_batch, world, rank)
    ctrl.set_ik(first_robot=lo, **kwargs)


def end_episodes(ctrl, world, rank, done, extra, bit=64):
    """Controller.end_episodes on this rank's shard of done and extra given for the whole batch (numpy): the shard's slice of
    done is updated in place"""
    lo, hi = shard_bounds(done.shape[0], world, rank)
    ctrl.end_episodes(done[lo:hi], shard_rows(extra, world, rank), bit)


def reinitialize_robots(ctrl, world, rank, mask, task=-1):
    """Controller.reinitialize_robots on this rank's shard of a mask given for the whole batch"""
    ctrl.reinitialize_robots(shard_rows(mask, world, rank), task)


def reset_robots(ctrl, world, rank, mask, q=None, dq=None):
    """Controller.reset_robots on this rank's shard of a mask and state rows given for the whole batch"""
    ctrl.reset_robots(*[shard_rows(a, world, rank) for a in (mask, q, dq)])


def set_reset_sampler(ctrl, world, rank, global_batch, rows=None, first_robot=0, **kwargs):
    """Controller.set_reset_sampler on this rank's shard of the per-robot rows [total][global_batch] given for the whole batch
    (None: the defaults), with first_robot (the whole batch's: its robot 0) moved on by the shard's first global index: every
    robot draws the start state and the goals it draws in the one-context run"""
    lo, _ = shard_bounds(global_batch, world, rank)
    ctrl.set_reset_sampler(rows=shard_rows(rows, world, rank), first_robot=int(first_robot) + lo, **kwargs)


def reset_robots_sampled(ctrl, world, rank, mask):
    """Controller.reset_robots_sampled on this rank's shard of a mask given for the whole batch"""
    ctrl.reset_robots_sampled(shard_rows(mask, world, rank))


def set_env_sampler(ctrl, world, rank, global_batch, first_robot=0, **kwargs):
    """Controller.set_env_sampler with first_robot (the whole batch's: its robot 0) moved on by the shard's first global index:
    every robot draws the plant it draws in the one-context run"""
    lo, _ = shard_bounds(global_batch, world, rank)
    ctrl.set_env_sampler(first_robot=int(first_robot) + lo, **kwargs)


def randomize_robots(ctrl, world, rank, mask, groups=0):
    """Controller.randomize_robots on this rank's shard of a mask given for the whole batch"""
    ctrl.randomize_robots(shard_rows(mask, world, rank), groups)


def observe(ctrl, world, rank, out=None, done=None):
    """Controller.observe on this rank's shard, written into this rank's columns [lo, hi) of host arrays given for the whole
    batch: out [rows][global_batch] float64, done [global_batch] uint8 (one of the two may be None: not wanted). -> (lo, hi)"""
    if out is None and done is None:
        raise ValueError("observe: give out, done or both (the arrays of the whole batch this rank's columns are written into)")
    lo, hi = shard_bounds((out if out is not None else done).shape[-1], world, rank)
    if hi - lo != ctrl.B:
        raise ValueError(f"rank {rank} owns {hi - lo} robots of the arrays given, its controller has {ctrl.B}")
    part_out, part_done = ctrl.observe(out=None if out is not None else False, done=None if done is not None else False)
    if out is not None:
        out[:, lo:hi] = part_out
    if done is not None:
        done[lo:hi] = part_done
    return lo, hi


def apply_action(ctrl, world, rank, action, mask=None):
    """Controller.apply_action on this rank's shard of an action [rows][global_batch] and mask [global_batch] given for the
    whole batch"""
    ctrl.apply_action(shard_rows(action, world, rank), shard_rows(mask, world, rank))


def node_throughput(robots_per_rank, world, steps, elapsed_max):
    """whole-job control-ticks/sec: every rank's robots x steps over the slowest rank's time"""
    return robots_per_rank * world * steps / elapsed_max


def finalize():
    if dist.is_initialized():
        dist.destroy_process_group()

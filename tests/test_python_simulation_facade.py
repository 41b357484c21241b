"""The members of the Python BatchedSimulation that forward to the Controller: joint dynamics (setJointDynamics,
clearJointDynamics, getJointDynamicsState) and the contact members the C++ facade has (setContactPlanes, clearContact,
attachForceSensor, detachForceSensor, getContactState, robotsInContact). On the CPU: they exist and forward, argument for
argument, to a recording stand-in. On the GPU: one period through the facade is bit-equal to the same period through
Controller."""
import numpy as np
import pytest

import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi


class _Recorder:
    """stands where the Controller does: records every call"""

    def __init__(self):
        self.calls = []
        cfg = _abi.ContactConfig()
        cfg.n_points, cfg.link, cfg.sensor_task = 1, 6, -1
        self._contact = (cfg, np.arange(9.0 * 3).reshape(9, 3))

    def get_contact(self):
        return self._contact

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
            return name

        return call


class _Owner:
    def __init__(self, ctrl):
        self._ctrl = ctrl


def test_members_exist_and_forward():
    rec = _Recorder()
    sim = pkg.BatchedSimulation(_Owner(rec), 0.001, 3)
    sim.setJointDynamics(armature=0.1, torque_limit="model", stop_stiffness=1e4)
    sim.clearJointDynamics()
    assert sim.getJointDynamicsState() == "get_joint_dynamics_state"
    sim.setContactPlanes(6, [[0, 0, 0.1]], "p", "n", "k", damping="d", sensor_task=0)
    sim.clearContact()
    assert sim.getContactState() == "get_contact_state" and sim.robotsInContact() == "robots_in_contact"
    assert rec.calls == [("set_joint_dynamics", (), dict(armature=0.1, torque_limit="model", stop_stiffness=1e4)), ("clear_joint_dynamics", (), {}),
                         ("get_joint_dynamics_state", (), {}), ("set_contact", (6, [[0, 0, 0.1]], "p", "n", "k"), dict(damping="d", sensor_task=0)),
                         ("clear_contact", (), {}), ("get_contact_state", (), {}), ("robots_in_contact", (), {})]
    # the sensor: the contact in force, sent again with the task's index (-1: detached)
    for member, task in ((lambda: sim.attachForceSensor(0), 0), (sim.detachForceSensor, -1)):
        rec.calls.clear()
        member()
        (name, a, kw), = rec.calls
        assert name == "set_contact" and a[0] is rec.get_contact()[0] and a[0].sensor_task == task and a[1] is None and not kw
        rows = rec.get_contact()[1]
        assert all(np.array_equal(x, y) for x, y in zip(a[2:], (rows[0:3], rows[3:6], rows[6], rows[7], rows[8])))
    rec._contact[0].n_points = 0
    with pytest.raises(ValueError, match="no contact is set"):
        sim.attachForceSensor(0)


@pytest.mark.gpu
def test_one_period_through_the_facade_is_the_controllers():
    import joint_dynamics_cases as jc

    B = 65
    case = jc.draw("panda", B)
    rows, k = jc.select(case, "all")
    kw = jc.keywords(rows, k)
    robot = pkg.BatchedRobotModel(B)
    robot.setQ(case["q"])
    robot.setDq(case["dq"])
    rc = pkg.RobotController(robot, [pkg.JointTask(robot)])
    sim = pkg.BatchedSimulation(rc, jc.DT, jc.SUBSTEPS)
    sim.enableGravity(True)
    sim.setJointDynamics(**kw)
    rc._ctrl.set_state(case["q"], case["dq"])
    sim.setJointTorques(case["tau"])
    sim.integrate()
    g = pkg.Controller(pkg.panda_model(), [pkg.joint_task_config("j")], B)
    g.set_joint_dynamics(**kw)
    g.set_state(case["q"], case["dq"])
    g.sim_step(case["tau"], jc.DT, jc.SUBSTEPS, True)
    q, dq = g.get_state()
    assert np.array_equal(sim.getJointPositions(), q) and np.array_equal(sim.getJointVelocities(), dq)
    a, b = sim.getJointDynamicsState(), g.get_joint_dynamics_state()
    assert all(np.array_equal(a[key], b[key]) for key in b) and b["robots_saturated"] > B // 2
    sim.clearJointDynamics()
    g.clear_joint_dynamics()
    for c in (rc._ctrl, g):
        c.set_state(case["q"], case["dq"])
    sim.setJointTorques(case["tau"])
    sim.integrate()
    g.sim_step(case["tau"], jc.DT, jc.SUBSTEPS, True)
    assert np.array_equal(sim.getJointPositions(), g.get_state()[0])

// The joint-dynamics members of BatchedSimulation (include/Sai2PrimitivesBatched.h) compile against the C ABI, and the checks
// that setJointDynamics makes ahead of the device (BatchedSimulation::checkJointDynamicsArguments: every condition
// sai2b_set_joint_dynamics puts on host arguments, plus the shapes) throw std::invalid_argument.
// Usage: joint_dynamics_facade_test validate
#include <cstdio>
#include <cstring>
#include <functional>

#include "Sai2PrimitivesBatched.h"

using namespace Sai2Primitives;

static int failures = 0;
static void expect_invalid(const char* what, const std::function<void()>& f) {
	try {
		f();
	} catch (const std::invalid_argument& e) {
		std::printf("ok   %s: %s\n", what, e.what());
		return;
	} catch (const std::exception& e) {
		std::printf("FAIL %s: threw %s\n", what, e.what());
		failures++;
		return;
	}
	std::printf("FAIL %s: did not throw\n", what);
	failures++;
}

int main(int argc, char** argv) {
	if (argc < 2 || std::strcmp(argv[1], "validate") != 0) {
		std::fprintf(stderr, "usage: %s validate\n", argv[0]);
		return 2;
	}
	using JD = BatchedSimulation::JointDynamics;
	// the members exist with these signatures (never called: there is no device here)
	void (BatchedSimulation::*set)(const JD&) = &BatchedSimulation::setJointDynamics;
	void (BatchedSimulation::*from_model)(const BatchedRobotModel&) = &BatchedSimulation::setJointDynamicsFromModel;
	void (BatchedSimulation::*from_model_with)(const BatchedRobotModel&, JD) = &BatchedSimulation::setJointDynamicsFromModel;
	void (BatchedSimulation::*clear)() = &BatchedSimulation::clearJointDynamics;
	BatchedSimulation::JointDynamicsState (BatchedSimulation::*state)() const = &BatchedSimulation::getJointDynamicsState;
	int (BatchedSimulation::*saturated)() const = &BatchedSimulation::robotsSaturated;
	int (BatchedSimulation::*at_stop)() const = &BatchedSimulation::robotsAtStop;
	if (!set || !from_model || !from_model_with || !clear || !state || !saturated || !at_stop) return 3;
	if (sai2b_sizeof_joint_dynamics_config() != (int)sizeof(sai2b_joint_dynamics_config)) return 4;

	// the checks setJointDynamics makes before it touches the device, on a two-robot batch of a 7-joint robot
	const int dof = 7;
	const size_t B = 2, NB = dof * B;
	JD ok;
	ok.armature = Batch(NB, 0.1), ok.damping = Batch(NB, 1.0), ok.friction = Batch(NB, 0.5), ok.torque_limit = Batch(NB, 20.0);
	ok.q_lower = Batch(NB, -2.0), ok.q_upper = Batch(NB, 2.0);
	ok.stop_stiffness = {1e4}, ok.stop_damping = {0.5}, ok.friction_velocity_eps = std::vector<double>(dof, 1e-3);
	auto check = [&](const JD& jd) { BatchedSimulation::checkJointDynamicsArguments(dof, B, jd); };
	check(ok);		// accepted
	check(JD());	// nothing set: accepted
	auto with = [&](const std::function<void(JD&)>& edit) {
		JD jd = ok;
		edit(jd);
		return jd;
	};
	check(with([](JD& j) { j.torque_limit[3] = INFINITY, j.q_lower[2] = -INFINITY, j.q_upper[5] = INFINITY; }));  // allowed infinities
	expect_invalid("row of the wrong size", [&] { check(with([](JD& j) { j.damping = Batch(3, 0.0); })); });
	expect_invalid("two stop stiffnesses", [&] { check(with([](JD& j) { j.stop_stiffness = {1.0, 2.0}; })); });
	expect_invalid("negative armature", [&] { check(with([](JD& j) { j.armature[4] = -1e-3; })); });
	expect_invalid("non-finite armature", [&] { check(with([](JD& j) { j.armature[4] = INFINITY; })); });
	expect_invalid("negative damping", [&] { check(with([](JD& j) { j.damping[1] = -0.1; })); });
	expect_invalid("NaN damping", [&] { check(with([](JD& j) { j.damping[1] = NAN; })); });
	expect_invalid("negative friction", [&] { check(with([](JD& j) { j.friction[13] = -0.1; })); });
	expect_invalid("torque limit 0", [&] { check(with([](JD& j) { j.torque_limit[0] = 0.0; })); });
	expect_invalid("NaN torque limit", [&] { check(with([](JD& j) { j.torque_limit[0] = NAN; })); });
	expect_invalid("NaN lower limit", [&] { check(with([](JD& j) { j.q_lower[6] = NAN; })); });
	expect_invalid("NaN upper limit", [&] { check(with([](JD& j) { j.q_upper[6] = NAN; })); });
	expect_invalid("lower == upper", [&] { check(with([](JD& j) { j.q_lower[7] = 2.0; })); });
	expect_invalid("lower above upper", [&] { check(with([](JD& j) { j.q_upper[7] = -3.0; })); });
	expect_invalid("lower +inf, no upper", [&] { check(with([](JD& j) { j.q_upper.clear(), j.q_lower[7] = INFINITY; })); });
	expect_invalid("negative stop stiffness", [&] { check(with([](JD& j) { j.stop_stiffness = {-1.0}; })); });
	expect_invalid("non-finite stop damping", [&] { check(with([](JD& j) { j.stop_damping = {INFINITY}; })); });
	expect_invalid("friction_velocity_eps 0", [&] { check(with([](JD& j) { j.friction_velocity_eps[2] = 0.0; })); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

// The observation members of the C++ facade (include/Sai2PrimitivesBatched.h: setObservation, clearObservation,
// observationRows, observationLayout, observe, doneCounts on RobotController, BatchedSimulation and
// ShardedRobotController) compile against the C ABI, and the checks they make ahead of the device
// (detail::checkObservationConfig: sai2b_validate_observation against the hierarchy; detail::checkObserveArguments: the
// sizes of out and done) throw std::invalid_argument.
// Usage: observation_facade_test validate
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

template <class T>
static bool has_members() {
	void (T::*set)(const sai2b_observation_config&) = &T::setObservation;
	void (T::*clear)() = &T::clearObservation;
	int (T::*rows)() const = &T::observationRows;
	void (T::*observe)(Batch*, std::vector<unsigned char>*) = &T::observe;
	return set && clear && rows && observe;
}

int main(int argc, char** argv) {
	if (argc < 2 || std::strcmp(argv[1], "validate") != 0) {
		std::fprintf(stderr, "usage: %s validate\n", argv[0]);
		return 2;
	}
	// the members exist with these signatures (never called: there is no device here)
	if (!has_members<RobotController>() || !has_members<BatchedSimulation>() || !has_members<ShardedRobotController>()) return 3;
	std::pair<int, int> (RobotController::*layout)(int, int) const = &RobotController::observationLayout;
	Observation (BatchedSimulation::*observe_all)() = &BatchedSimulation::observe;
	DoneCounts (RobotController::*counts)() const = &RobotController::doneCounts;
	DoneCounts (ShardedRobotController::*sharded_counts)() = &ShardedRobotController::doneCounts;
	if (!layout || !observe_all || !counts || !sharded_counts) return 3;

	// the sizes observe(out, done) checks before it touches the device: 20 rows, 3 robots
	const size_t B = 3;
	Batch out(20 * B);
	std::vector<unsigned char> done(B);
	detail::checkObserveArguments(20, B, &out, &done);	// accepted
	detail::checkObserveArguments(20, B, nullptr, &done);
	detail::checkObserveArguments(20, B, &out, nullptr);
	detail::checkObserveArguments(0, B, nullptr, &done);  // criteria only
	expect_invalid("no observation configured", [&] { detail::checkObserveArguments(-1, B, &out, &done); });
	expect_invalid("out of the wrong size", [&] {
		Batch small(19 * B);
		detail::checkObserveArguments(20, B, &small, &done);
	});
	expect_invalid("done of the wrong size", [&] {
		std::vector<unsigned char> d(B + 1);
		detail::checkObserveArguments(20, B, &out, &d);
	});

	// the configuration against a hierarchy [MotionForceTask, JointTask] of the Panda
	std::vector<sai2b_task_config> tasks(2);
	sai2b_default_motion_force_task(&tasks[0], "m", 6, nullptr, nullptr, -1, nullptr, -1, nullptr);
	sai2b_default_joint_task(&tasks[1], "j", 0, nullptr);
	sai2b_observation_config ok;
	if (sai2b_default_observation(&ok) != SAI2B_OK || sai2b_sizeof_observation_config() != (int)sizeof(ok)) return 4;
	detail::checkObservationConfig(ok, tasks, SAI2B_DOF);  // the default: accepted
	ok.blocks = SAI2B_OBS_Q | SAI2B_OBS_LIMIT_MARGIN;
	ok.task_mask = 1, ok.task_blocks = SAI2B_OBS_POSE | SAI2B_OBS_ERROR;
	ok.criteria = SAI2B_DONE_SUCCESS | SAI2B_DONE_TIMEOUT, ok.success_task_mask = 1, ok.pos_tolerance = 1e-3, ok.ori_tolerance = 1e-2;
	ok.max_episode_steps = 100;
	detail::checkObservationConfig(ok, tasks, SAI2B_DOF);
	int first = 0, n = 0, total = 0;
	if (sai2b_observation_config_layout(&ok, SAI2B_DOF, SAI2B_OBS_ERROR, 0, &first, &n, &total) != SAI2B_OK || first != 20 || n != 8 || total != 28) return 5;
	auto with = [&](const std::function<void(sai2b_observation_config&)>& edit) {
		sai2b_observation_config c = ok;
		edit(c);
		return c;
	};
	expect_invalid("observed task is a JointTask", [&] { detail::checkObservationConfig(with([](auto& c) { c.task_mask = 2; }), tasks, SAI2B_DOF); });
	expect_invalid("success task past the tasks", [&] { detail::checkObservationConfig(with([](auto& c) { c.success_task_mask = 4; }), tasks, SAI2B_DOF); });
	expect_invalid("negative tolerance", [&] { detail::checkObservationConfig(with([](auto& c) { c.pos_tolerance = -1.0; }), tasks, SAI2B_DOF); });
	expect_invalid("non-finite margin", [&] { detail::checkObservationConfig(with([](auto& c) { c.joint_limit_margin = NAN; }), tasks, SAI2B_DOF); });
	expect_invalid("SUCCESS without a task", [&] { detail::checkObservationConfig(with([](auto& c) { c.success_task_mask = 0; }), tasks, SAI2B_DOF); });
	expect_invalid("TIMEOUT without steps", [&] { detail::checkObservationConfig(with([](auto& c) { c.max_episode_steps = 0; }), tasks, SAI2B_DOF); });
	expect_invalid("unknown block bits", [&] { detail::checkObservationConfig(with([](auto& c) { c.blocks = 128; }), tasks, SAI2B_DOF); });
	expect_invalid("unknown task block bits", [&] { detail::checkObservationConfig(with([](auto& c) { c.task_blocks = 32; }), tasks, SAI2B_DOF); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

// The masked re-initialisation and the episode reset through the C++ facade (include/Sai2PrimitivesBatched.h).
//   validate  no device: the members exist with the documented signatures, and the check they all make ahead of the device
//             (detail::checkResetArguments) throws std::invalid_argument for a wrong mask length or state size
//   run       257 robots over two uneven shards on device 0, a mask straddling the shard boundary, against one context of the
//             whole batch given the same mask through the C ABI: torques bit for bit over the periods after each call.
// Prints "ok <name>" per check and "<n> failures" at the end.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "Sai2PrimitivesBatched.h"

using namespace Sai2Primitives;
using Mask = std::vector<unsigned char>;

static int failures = 0;
static void check(bool ok, const char* name) {
	std::printf("%s %s\n", ok ? "ok" : "FAILED", name);
	if (!ok) failures++;
}
template <class F> static bool throws_invalid(F f) {
	try {
		f();
	} catch (const std::invalid_argument&) {
		return true;
	} catch (...) {
	}
	return false;
}

static std::vector<sai2b_task_config> hierarchy() {
	std::vector<sai2b_task_config> cfgs(2);
	const double fp[3] = {0, 0, 0.1};
	detail::check(nullptr, sai2b_default_motion_force_task(&cfgs[0], "mft", 6, fp, nullptr, -1, nullptr, -1, nullptr));
	detail::check(nullptr, sai2b_default_joint_task(&cfgs[1], "jt", 7, nullptr));
	for (int i = 0; i < 3; i++) cfgs[0].ki_pos[i] = 4.0, cfgs[0].ki_ori[i] = 2.0;
	for (int i = 0; i < 7; i++) cfgs[1].ki[i] = 3.0;
	return cfgs;  // (both generators on: the library default)
}

static int validate() {
	// the members, by signature
	static_assert(std::is_same<decltype(static_cast<void (RobotController::*)(const Mask&)>(&RobotController::reinitializeTasks)),
							   void (RobotController::*)(const Mask&)>::value, "RobotController::reinitializeTasks(mask)");
	static_assert(std::is_same<decltype(&RobotController::resetRobots), void (RobotController::*)(const Mask&, const Batch&, const Batch&)>::value,
				  "RobotController::resetRobots(mask, q, dq)");
	static_assert(std::is_same<decltype(static_cast<void (TemplateTask::*)(const Mask&)>(&TemplateTask::reInitializeTask)),
							   void (TemplateTask::*)(const Mask&)>::value, "TemplateTask::reInitializeTask(mask)");
	static_assert(std::is_same<decltype(static_cast<void (ShardedRobotController::*)(const Mask&)>(&ShardedRobotController::reinitializeTasks)),
							   void (ShardedRobotController::*)(const Mask&)>::value, "ShardedRobotController::reinitializeTasks(mask)");
	static_assert(std::is_same<decltype(&ShardedRobotController::reInitializeTask), void (ShardedRobotController::*)(int, const Mask&)>::value,
				  "ShardedRobotController::reInitializeTask(task, mask)");
	static_assert(std::is_same<decltype(&ShardedRobotController::resetRobots),
							   void (ShardedRobotController::*)(const Mask&, const Batch&, const Batch&)>::value,
				  "ShardedRobotController::resetRobots(mask, q, dq)");
	check(true, "members compile");
	const Mask m5(5, 1);
	const Batch q5(7 * 5, 0.0);
	detail::checkResetArguments(7, 5, m5, q5, q5, "accepted");
	detail::checkResetArguments(7, 5, m5, {}, {}, "accepted");
	check(throws_invalid([&] { detail::checkResetArguments(7, 5, Mask(4, 1), q5, q5, "f"); }), "mask too short");
	check(throws_invalid([&] { detail::checkResetArguments(7, 5, Mask(6, 1), {}, {}, "f"); }), "mask too long");
	check(throws_invalid([&] { detail::checkResetArguments(7, 5, Mask(), {}, {}, "f"); }), "empty mask");
	check(throws_invalid([&] { detail::checkResetArguments(7, 5, m5, Batch(7 * 5 - 1), {}, "f"); }), "q of the wrong size");
	check(throws_invalid([&] { detail::checkResetArguments(7, 5, m5, {}, Batch(7 * 4), "f"); }), "dq of the wrong size");
	check(throws_invalid([&] { detail::checkResetArguments(4, 5, m5, q5, {}, "f"); }), "q of another robot size");
	// the C entry points reject a NULL context before anything touches a device
	const Mask one(1, 1);
	check(sai2b_reinitialize_robots(nullptr, -1, one.data(), 0) != SAI2B_OK, "sai2b_reinitialize_robots(NULL ctx)");
	check(sai2b_reset_robots(nullptr, one.data(), nullptr, nullptr, 0) != SAI2B_OK, "sai2b_reset_robots(NULL ctx)");
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

static Batch gather(int dof, int B, sai2b_ctx* c) {
	Batch tau((size_t)dof * B);
	detail::check(c, sai2b_tick(c, tau.data(), 0));
	detail::check(c, sai2b_sim_step(c, nullptr, 0, 0.001, 1, 0));
	return tau;
}

static int run() {
	const int B = 257, n = 7;
	sai2b_robot_model model;
	detail::check(nullptr, sai2b_panda_model(&model));
	const std::vector<sai2b_task_config> cfgs = hierarchy();
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5};
	Batch q(n * (size_t)B), dq(n * (size_t)B), q1(n * (size_t)B), dq1(n * (size_t)B), goal(n * (size_t)B);
	for (int b = 0; b < B; b++)
		for (int i = 0; i < n; i++) {
			const size_t k = i * (size_t)B + b;
			q[k] = q0[i] + 0.3 * std::sin(0.37 * b + i), dq[k] = 0.2 * std::cos(0.11 * b + 2 * i);
			q1[k] = q0[i] + 0.25 * std::cos(0.23 * b + 2 * i), dq1[k] = 0.1 * std::sin(0.19 * b + i);
			goal[k] = q[k] + 0.1 * std::sin(0.7 * b + 3 * i);
		}
	ShardedRobotController sharded(model, cfgs, B, {0, 0});
	const int cut = sharded.shardBounds(0).second;
	check(cut != B - cut && sharded.shardBounds(1).first == cut, "two uneven shards");
	Mask mask(B, 0);
	for (int b : {0, 63, cut - 2, cut - 1, cut, cut + 1, 200, B - 1}) mask[b] = 1;  // straddles the boundary
	// size checks of every facade that owns contexts
	check(throws_invalid([&] { sharded.reinitializeTasks(Mask(B - 1, 1)); }), "sharded reinitializeTasks: wrong mask length");
	check(throws_invalid([&] { sharded.reInitializeTask(0, Mask(B + 1, 1)); }), "sharded reInitializeTask: wrong mask length");
	check(throws_invalid([&] { sharded.reInitializeTask(2, mask); }), "sharded reInitializeTask: no such task");
	check(throws_invalid([&] { sharded.resetRobots(Mask(1, 1), q1, dq1); }), "sharded resetRobots: wrong mask length");
	check(throws_invalid([&] { sharded.resetRobots(mask, Batch(n * (size_t)B - 1), dq1); }), "sharded resetRobots: wrong q size");
	{
		auto robot = std::make_shared<BatchedRobotModel>(5, model, 0);
		auto jt = std::make_shared<JointTask>(robot, "jt");
		std::vector<std::shared_ptr<TemplateTask>> tasks = {jt};
		RobotController rc(robot, tasks);
		check(throws_invalid([&] { rc.reinitializeTasks(Mask(4, 1)); }), "RobotController reinitializeTasks: wrong mask length");
		check(throws_invalid([&] { rc.resetRobots(Mask(6, 1), Batch(), Batch()); }), "RobotController resetRobots: wrong mask length");
		check(throws_invalid([&] { rc.resetRobots(Mask(5, 1), Batch(3), Batch()); }), "RobotController resetRobots: wrong q size");
		check(throws_invalid([&] { jt->reInitializeTask(Mask(4, 1)); }), "JointTask reInitializeTask: wrong mask length");
		rc.resetRobots(Mask(5, 1), Batch(), Batch());
		rc.reinitializeTasks(Mask(5, 0));
		jt->reInitializeTask(Mask(5, 1));
		rc.tick();
		check(true, "RobotController members run");
	}
	// one context of the whole batch, the same script through the C ABI
	sai2b_ctx* one = sai2b_create(&model, cfgs.data(), (int)cfgs.size(), B, 0);
	if (!one) throw std::runtime_error(sai2b_last_error(nullptr));
	detail::check(one, sai2b_set_state(one, q.data(), dq.data(), 0));
	detail::check(one, sai2b_reinitialize(one));
	detail::check(one, sai2b_set_jt_goals(one, 1, goal.data(), nullptr, nullptr, 0));
	sharded.setState(q, dq);
	sharded.reinitializeTasks();
	sharded.setJointTaskGoals(1, goal);
	auto period_sharded = [&] {
		Batch tau((size_t)n * B);
		for (int s = 0; s < 2; s++) {
			const int lo = sharded.shardBounds(s).first, hi = sharded.shardBounds(s).second;
			const Batch part = gather(n, hi - lo, sharded.ctx(s));
			for (int c = 0; c < n; c++) std::copy(part.begin() + c * (size_t)(hi - lo), part.begin() + (c + 1) * (size_t)(hi - lo), tau.begin() + c * (size_t)B + lo);
		}
		return tau;
	};
	auto same = [&](int periods) {
		bool ok = true;
		for (int k = 0; k < periods; k++) {
			const Batch a = period_sharded(), b = gather(n, B, one);
			ok = ok && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
		}
		return ok;
	};
	check(same(20), "history bit-equal");
	sharded.resetRobots(mask, q1, dq1);
	detail::check(one, sai2b_reset_robots(one, mask.data(), q1.data(), dq1.data(), 0));
	check(same(10), "resetRobots bit-equal to one context");
	sharded.reInitializeTask(1, mask);
	detail::check(one, sai2b_reinitialize_robots(one, 1, mask.data(), 0));
	check(same(5), "reInitializeTask(task, mask) bit-equal to one context");
	sharded.reinitializeTasks(mask);
	detail::check(one, sai2b_reinitialize_robots(one, -1, mask.data(), 0));
	check(same(5), "reinitializeTasks(mask) bit-equal to one context");
	sai2b_destroy(one);
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

int main(int argc, char** argv) {
	try {
		if (argc > 1 && std::strcmp(argv[1], "validate") == 0) return validate();
		if (argc > 1 && std::strcmp(argv[1], "run") == 0) return run();
	} catch (const std::exception& e) {
		std::printf("exception: %s\n", e.what());
		return 3;
	}
	std::printf("usage: subset_reset_test validate|run\n");
	return 2;
}

// The action members of the C++ facade (include/Sai2PrimitivesBatched.h: setAction, clearAction, actionRows, actionLayout,
// applyAction, actionCounts on RobotController, BatchedSimulation and ShardedRobotController) against the C ABI.
//   validate  no device: the members exist, and the checks they make ahead of the device (detail::checkActionConfig:
//             sai2b_validate_action against the hierarchy; detail::checkActionArguments: the sizes of action and mask)
//             throw std::invalid_argument
//   run       on the GPU: 257 robots over two uneven shards, a mask that straddles the boundary, bit-equal to one context
//             of the whole batch (goal rows read back, counts summed, the next ticks' torques)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>

#include "Sai2PrimitivesBatched.h"

using namespace Sai2Primitives;

static int failures = 0;
static void check(bool ok, const char* what) {
	std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
	if (!ok) failures++;
}
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
	void (T::*set)(const sai2b_action_config&) = &T::setAction;
	void (T::*clear)() = &T::clearAction;
	int (T::*rows)() const = &T::actionRows;
	void (T::*apply)(const Batch&, const std::vector<unsigned char>&) = &T::applyAction;
	return set && clear && rows && apply;
}

static std::vector<sai2b_task_config> hierarchy() {
	std::vector<sai2b_task_config> tasks(2);
	const double fp[3] = {0, 0, 0.1};
	detail::check(nullptr, sai2b_default_motion_force_task(&tasks[0], "m", 6, fp, nullptr, -1, nullptr, -1, nullptr));
	detail::check(nullptr, sai2b_default_joint_task(&tasks[1], "j", 0, nullptr));
	tasks[0].use_internal_otg = tasks[1].use_internal_otg = 0;
	return tasks;
}

// position and orientation deltas from the robot as it is, joint deltas on the goal; clipping, a lead and a joint clamp
static sai2b_action_config configuration() {
	sai2b_action_config c;
	detail::check(nullptr, sai2b_default_action(&c));
	c.clip_actions = 1;
	c.task[0].mode = SAI2B_ACT_DELTA_CURRENT, c.task[0].blocks = SAI2B_ACT_POSITION | SAI2B_ACT_ORIENTATION;
	for (int k = 0; k < 3; k++) c.task[0].pos_scale[k] = 0.05;
	c.task[0].ori_scale = 0.3, c.task[0].max_pos_lead = 0.04;
	c.task[1].mode = SAI2B_ACT_DELTA_GOAL;
	for (int i = 0; i < 7; i++) c.task[1].jt_scale[i] = 0.1, c.task[1].jt_upper[i] = 2.0 + 0.1 * i;
	return c;
}

static int validate() {
	if (!has_members<RobotController>() || !has_members<BatchedSimulation>() || !has_members<ShardedRobotController>()) return 3;
	std::pair<int, int> (RobotController::*layout)(int, int) const = &RobotController::actionLayout;
	ActionCounts (RobotController::*counts)() const = &RobotController::actionCounts;
	ActionCounts (ShardedRobotController::*sharded_counts)() = &ShardedRobotController::actionCounts;
	if (!layout || !counts || !sharded_counts) return 3;
	const size_t B = 3;
	const Batch action(13 * B);
	detail::checkActionArguments(13, B, action, {});
	detail::checkActionArguments(13, B, action, std::vector<unsigned char>(B, 1));
	expect_invalid("no action configured", [&] { detail::checkActionArguments(-1, B, action, {}); });
	expect_invalid("action of the wrong size", [&] { detail::checkActionArguments(12, B, action, {}); });
	expect_invalid("mask of the wrong size", [&] { detail::checkActionArguments(13, B, action, std::vector<unsigned char>(B + 1, 1)); });
	const std::vector<sai2b_task_config> tasks = hierarchy();
	const sai2b_action_config ok = configuration();
	if (sai2b_sizeof_action_config() != (int)sizeof(ok)) return 4;
	detail::checkActionConfig(ok, tasks, SAI2B_DOF);
	int first = 0, n = 0, total = 0;
	if (sai2b_action_config_layout(&ok, tasks.data(), 2, SAI2B_ACT_ORIENTATION, 0, &first, &n, &total) != SAI2B_OK || first != 3 || n != 3 || total != 13) return 5;
	if (sai2b_action_config_layout(&ok, tasks.data(), 2, 0, 1, &first, &n, &total) != SAI2B_OK || first != 6 || n != 7) return 5;
	auto with = [&](const std::function<void(sai2b_action_config&)>& edit) {
		sai2b_action_config c = ok;
		edit(c);
		return c;
	};
	expect_invalid("default: no task has a mode", [&] {
		sai2b_action_config c;
		sai2b_default_action(&c);
		detail::checkActionConfig(c, tasks, SAI2B_DOF);
	});
	expect_invalid("unknown mode", [&] { detail::checkActionConfig(with([](auto& c) { c.task[0].mode = 7; }), tasks, SAI2B_DOF); });
	expect_invalid("blocks on a JointTask", [&] { detail::checkActionConfig(with([](auto& c) { c.task[1].blocks = 1; }), tasks, SAI2B_DOF); });
	expect_invalid("no block", [&] { detail::checkActionConfig(with([](auto& c) { c.task[0].blocks = 0; }), tasks, SAI2B_DOF); });
	expect_invalid("task past the tasks", [&] { detail::checkActionConfig(with([](auto& c) { c.task[3].mode = 1; }), tasks, SAI2B_DOF); });
	expect_invalid("negative scale", [&] { detail::checkActionConfig(with([](auto& c) { c.task[0].ori_scale = -1.0; }), tasks, SAI2B_DOF); });
	expect_invalid("empty box", [&] { detail::checkActionConfig(with([](auto& c) { c.task[0].pos_lower[1] = 1.0, c.task[0].pos_upper[1] = 1.0; }), tasks, SAI2B_DOF); });
	expect_invalid("zero lead", [&] { detail::checkActionConfig(with([](auto& c) { c.task[0].max_pos_lead = 0.0; }), tasks, SAI2B_DOF); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

static Batch goals_of(sai2b_ctx* c, int B) {  // position 3, rotation 9, joint goal 7
	Batch g(19 * (size_t)B);
	detail::check(c, sai2b_get_mft_goals(c, 0, g.data(), g.data() + 3 * (size_t)B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
	detail::check(c, sai2b_get_jt_goals(c, 1, g.data() + 12 * (size_t)B, nullptr, nullptr));
	return g;
}

static int run() {
	const int B = 257, n = 7, R = 13;
	sai2b_robot_model model;
	detail::check(nullptr, sai2b_panda_model(&model));
	const std::vector<sai2b_task_config> cfgs = hierarchy();
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5};
	Batch q(n * (size_t)B), dq(n * (size_t)B), action(R * (size_t)B);
	for (int b = 0; b < B; b++) {
		for (int i = 0; i < n; i++) q[i * (size_t)B + b] = q0[i] + 0.3 * std::sin(0.37 * b + i), dq[i * (size_t)B + b] = 0.2 * std::cos(0.11 * b + 2 * i);
		for (int r = 0; r < R; r++) action[r * (size_t)B + b] = 1.4 * std::sin(0.53 * b + 1.7 * r);
	}
	ShardedRobotController sharded(model, cfgs, B, {0, 0});
	const int cut = sharded.shardBounds(0).second;
	check(cut != B - cut && sharded.shardBounds(1).first == cut, "two uneven shards");
	action[2 * (size_t)B + 5] = NAN, action[7 * (size_t)B + cut] = INFINITY;  // one rejected robot per shard
	std::vector<unsigned char> mask(B, 1);
	for (int b : {1, 64, cut - 1, cut + 1, B - 2}) mask[b] = 0;
	sai2b_ctx* one = sai2b_create(&model, cfgs.data(), (int)cfgs.size(), B, 0);
	if (!one) throw std::runtime_error(sai2b_last_error(nullptr));
	detail::check(one, sai2b_set_state(one, q.data(), dq.data(), 0));
	detail::check(one, sai2b_reinitialize(one));
	sharded.setState(q, dq);
	sharded.reinitializeTasks();
	expect_invalid("sharded applyAction before setAction", [&] { sharded.applyAction(action); });
	const sai2b_action_config cfg = configuration();
	sharded.setAction(cfg);
	detail::check(one, sai2b_set_action(one, &cfg));
	check(sharded.actionRows() == R && sai2b_action_rows(one) == R, "13 rows");
	expect_invalid("sharded applyAction: wrong action size", [&] { sharded.applyAction(Batch(R * (size_t)B - 1)); });
	expect_invalid("sharded applyAction: wrong mask size", [&] { sharded.applyAction(action, std::vector<unsigned char>(B - 1, 1)); });
	auto same = [&](const char* what) {
		Batch a(19 * (size_t)B);
		for (int s = 0; s < 2; s++) {
			const int lo = sharded.shardBounds(s).first, hi = sharded.shardBounds(s).second;
			const Batch part = goals_of(sharded.ctx(s), hi - lo);
			for (int c = 0; c < 19; c++) std::copy(part.begin() + c * (size_t)(hi - lo), part.begin() + (c + 1) * (size_t)(hi - lo), a.begin() + c * (size_t)B + lo);
		}
		const Batch b = goals_of(one, B);
		int c1[3];
		detail::check(one, sai2b_get_action_counts(one, c1));
		const ActionCounts cs = sharded.actionCounts();
		std::printf("     counts: rejected %d clipped %d limited %d\n", c1[0], c1[1], c1[2]);
		check(std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0, what);
		check(cs.rejected == c1[0] && cs.clipped == c1[1] && cs.limited == c1[2], "counts summed over the shards");
		return c1[0];
	};
	for (int k = 0; k < 2; k++) {  // twice: the joint deltas accumulate
		sharded.applyAction(action, mask);
		detail::check(one, sai2b_apply_action(one, action.data(), mask.data(), 0));
		check(same("masked applyAction bit-equal to one context") == 2, "one rejected robot per shard");
	}
	sharded.applyAction(action);
	detail::check(one, sai2b_apply_action(one, action.data(), nullptr, 0));
	same("applyAction of every robot bit-equal to one context");
	Batch tau_one((size_t)n * B);
	detail::check(one, sai2b_tick(one, tau_one.data(), 0));
	const Batch tau = sharded.tick();
	check(std::memcmp(tau.data(), tau_one.data(), tau.size() * sizeof(double)) == 0, "next tick bit-equal");
	sharded.clearAction();
	check(sharded.actionRows() == -1, "cleared");
	{
		auto robot = std::make_shared<BatchedRobotModel>(5, model, 0);
		auto jt = std::make_shared<JointTask>(robot, "jt");
		std::vector<std::shared_ptr<TemplateTask>> tasks = {jt};
		RobotController rc(robot, tasks);
		BatchedSimulation sim(rc);
		sai2b_action_config c;
		sai2b_default_action(&c);
		c.task[0].mode = SAI2B_ACT_ABSOLUTE;
		expect_invalid("RobotController applyAction before setAction", [&] { rc.applyAction(Batch(35)); });
		rc.setAction(c);
		check(sim.actionRows() == 7 && rc.actionLayout(0, 0) == std::make_pair(0, 7), "RobotController and BatchedSimulation share the configuration");
		Batch a(35);
		for (size_t i = 0; i < a.size(); i++) a[i] = 0.01 * (double)i;
		sim.applyAction(a, std::vector<unsigned char>{1, 1, 0, 1, 1});
		const Batch g = jt->getGoalPosition();
		bool ok = true;
		for (int i = 0; i < 7; i++)
			for (int b = 0; b < 5; b++) ok = ok && (b == 2 || g[i * 5 + b] == a[i * 5 + b]);
		check(ok && g[2] != a[2] && rc.actionCounts().rejected == 0, "absolute joint goals through the facade");
		rc.clearAction();
		check(rc.actionRows() == -1, "RobotController cleared");
	}
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
	std::printf("usage: action_facade_test validate|run\n");
	return 2;
}

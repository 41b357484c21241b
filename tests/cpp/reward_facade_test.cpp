// The reward members of the C++ facade (include/Sai2PrimitivesBatched.h: setReward, clearReward, rewardRows, rewardLayout,
// observeReward, rewardCounts, episodeStats on detail::ObservationMembers, which RobotController and BatchedSimulation share)
// against the C ABI.
//   reward_facade_test validate   no device: the members exist, the checks ahead of the device throw std::invalid_argument
//   reward_facade_test run        six periods tick -> integrate -> observeReward through the facade, bit-equal to the same
//                                 periods through sai2b_tick / sai2b_sim_step / sai2b_observe_reward on a twin; clearReward; the
//                                 exceptions for wrong sizes on a live controller
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
	void (T::*set)(const sai2b_reward_config&) = &T::setReward;
	void (T::*clear)() = &T::clearReward;
	int (T::*rows)() const = &T::rewardRows;
	int (T::*layout)(int, int) const = &T::rewardLayout;
	void (T::*observe)(Batch*, std::vector<unsigned char>*, std::vector<double>*, Batch*) = &T::observeReward;
	RewardCounts (T::*counts)() const = &T::rewardCounts;
	EpisodeStats (T::*stats)() const = &T::episodeStats;
	return set && clear && rows && layout && observe && counts && stats;
}

// every global term, and the position, velocity and force terms of task 0
static sai2b_reward_config configuration() {
	sai2b_reward_config c;
	sai2b_default_reward(&c);
	c.terms = SAI2B_REW_ALIVE | SAI2B_REW_JOINT_SPEED | SAI2B_REW_TORQUE | SAI2B_REW_TORQUE_RATE | SAI2B_REW_LIMIT | SAI2B_REW_DONE;
	const double w[SAI2B_REWARD_TERMS] = {0.25, -0.01, -1e-4, -1e-3, -3.0, 1.0};
	for (int k = 0; k < SAI2B_REWARD_TERMS; k++) c.weight[k] = w[k];
	c.task_mask = 1;
	c.task_terms = SAI2B_REW_POS_SQ | SAI2B_REW_ORI_TANH | SAI2B_REW_LIN_VEL_SQ | SAI2B_REW_FORCE_ERR_SQ | SAI2B_REW_FORCE_EXCESS;
	c.task_weight[0][1] = -2.0, c.task_weight[0][5] = 0.5, c.task_weight[0][6] = -0.05, c.task_weight[0][8] = -0.003, c.task_weight[0][9] = -0.1;
	c.done_value[5] = 0.125, c.done_value[2] = -2.5;
	c.limit_soft_margin = 0.3, c.ori_scale[0] = 0.4, c.force_soft_limit[0] = 2.0;
	c.gamma = 0.9, c.nonfinite_reward = -123.0;
	return c;
}

static int validate() {
	if (!has_members<RobotController>() || !has_members<BatchedSimulation>()) return 3;
	// the sizes observeReward checks before it touches the device: 11 term rows, 3 robots
	const size_t B = 3;
	std::vector<double> reward(B);
	Batch terms(11 * B);
	detail::checkRewardArguments(11, B, &reward, &terms);  // accepted
	detail::checkRewardArguments(11, B, nullptr, &terms);
	detail::checkRewardArguments(11, B, &reward, nullptr);
	detail::checkRewardArguments(11, B, nullptr, nullptr);
	expect_invalid("no reward configured", [&] { detail::checkRewardArguments(-1, B, &reward, &terms); });
	expect_invalid("reward of the wrong size", [&] {
		std::vector<double> r(B - 1);
		detail::checkRewardArguments(11, B, &r, &terms);
	});
	expect_invalid("terms of the wrong size", [&] {
		Batch t(10 * B);
		detail::checkRewardArguments(11, B, &reward, &t);
	});
	// the configuration against a hierarchy [MotionForceTask, JointTask] of the Panda
	std::vector<sai2b_task_config> tasks(2);
	sai2b_default_motion_force_task(&tasks[0], "m", 6, nullptr, nullptr, -1, nullptr, -1, nullptr);
	sai2b_default_joint_task(&tasks[1], "j", 0, nullptr);
	const sai2b_reward_config ok = configuration();
	if (sai2b_sizeof_reward_config() != (int)sizeof(ok)) return 4;
	detail::checkRewardConfig(ok, tasks, SAI2B_DOF);
	int first = 0, n = 0, total = 0;
	if (sai2b_reward_config_layout(&ok, SAI2B_REW_FORCE_ERR_SQ, 0, &first, &n, &total) != SAI2B_OK || first != 9 || n != 1 || total != 11) return 5;
	auto with = [&](const std::function<void(sai2b_reward_config&)>& edit) {
		sai2b_reward_config c = ok;
		edit(c);
		return c;
	};
	expect_invalid("task is a JointTask", [&] { detail::checkRewardConfig(with([](auto& c) { c.task_mask = 2; }), tasks, SAI2B_DOF); });
	expect_invalid("task terms without a task", [&] { detail::checkRewardConfig(with([](auto& c) { c.task_mask = 0; }), tasks, SAI2B_DOF); });
	expect_invalid("a task without task terms", [&] { detail::checkRewardConfig(with([](auto& c) { c.task_terms = 0; }), tasks, SAI2B_DOF); });
	expect_invalid("unknown term bits", [&] { detail::checkRewardConfig(with([](auto& c) { c.terms = 64; }), tasks, SAI2B_DOF); });
	expect_invalid("non-finite weight", [&] { detail::checkRewardConfig(with([](auto& c) { c.weight[2] = NAN; }), tasks, SAI2B_DOF); });
	expect_invalid("zero scale under TANH", [&] { detail::checkRewardConfig(with([](auto& c) { c.ori_scale[0] = 0.0; }), tasks, SAI2B_DOF); });
	expect_invalid("gamma above 1", [&] { detail::checkRewardConfig(with([](auto& c) { c.gamma = 1.5; }), tasks, SAI2B_DOF); });
	expect_invalid("no term", [&] { detail::checkRewardConfig(with([](auto& c) { c.terms = c.task_terms = c.task_mask = 0; }), tasks, SAI2B_DOF); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
	return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

static int run() {
	const int B = 130, n = 7;
	sai2b_robot_model model;
	detail::check(nullptr, sai2b_panda_model(&model));
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5}, frame[3] = {0.0, 0.0, 0.1};
	Batch q(n * (size_t)B), dq(n * (size_t)B), force(3 * (size_t)B), zero3(3 * (size_t)B, 0.0);
	for (int b = 0; b < B; b++) {
		for (int i = 0; i < n; i++) q[i * (size_t)B + b] = q0[i] + 0.3 * std::sin(0.37 * b + i), dq[i * (size_t)B + b] = 0.2 * std::cos(0.11 * b + 2 * i);
		for (int a = 0; a < 3; a++) force[a * (size_t)B + b] = 3.0 * std::sin(0.29 * b + a);
	}
	// two controllers built alike: `rc` is driven through the facade's members, `twin` through the C ABI on its context
	struct Rig {
		std::shared_ptr<BatchedRobotModel> robot;
		std::shared_ptr<MotionForceTask> mft;
		std::shared_ptr<JointTask> jt;
		std::unique_ptr<RobotController> rc;
	};
	auto build = [&]() {
		Rig r;
		r.robot = std::make_shared<BatchedRobotModel>(B, model, 0);
		r.robot->setQ(q), r.robot->setDq(dq);
		r.mft = std::make_shared<MotionForceTask>(r.robot, 6, frame, nullptr, "mft", true);
		const double axis[3] = {0.0, 0.0, 1.0};
		r.mft->parametrizeForceMotionSpaces(1, axis);
		r.jt = std::make_shared<JointTask>(r.robot, "jt");
		std::vector<std::shared_ptr<TemplateTask>> tasks = {r.mft, r.jt};
		r.rc = std::make_unique<RobotController>(r.robot, tasks);
		r.mft->setGoalForce(force);
		r.mft->updateSensedForceAndMoment(zero3, zero3);
		return r;
	};
	Rig a = build(), t = build();
	RobotController& rc = *a.rc;
	sai2b_ctx* twin = t.rc->ctx();
	BatchedSimulation sim(rc);
	sai2b_observation_config obs;
	sai2b_default_observation(&obs);
	obs.blocks = SAI2B_OBS_Q | SAI2B_OBS_EPISODE_STEP, obs.task_mask = 1, obs.task_blocks = SAI2B_OBS_ERROR;
	obs.criteria = SAI2B_DONE_SPEED | SAI2B_DONE_TIMEOUT, obs.max_episode_steps = 4;
	for (int i = 0; i < SAI2B_MAX_DOF; i++) obs.max_joint_speed[i] = 0.6;
	const sai2b_reward_config cfg = configuration();
	expect_invalid("setReward before setObservation", [&] { rc.setReward(cfg); });
	check(rc.rewardRows() == -1, "no reward yet");
	rc.setObservation(obs);
	detail::check(twin, sai2b_set_observation(twin, &obs));
	expect_invalid("observeReward before setReward", [&] { rc.observeReward(nullptr, nullptr, nullptr, nullptr); });
	rc.setReward(cfg);
	detail::check(twin, sai2b_set_reward(twin, &cfg));
	const int R = rc.observationRows(), T = rc.rewardRows();
	check(T == 11 && sim.rewardRows() == T && sai2b_reward_rows(twin) == T, "11 term rows, shared by RobotController and BatchedSimulation");
	check(rc.rewardLayout(SAI2B_REW_ALIVE) == 0 && rc.rewardLayout(SAI2B_REW_DONE) == 5 && rc.rewardLayout(SAI2B_REW_POS_SQ, 0) == 6 &&
			  sim.rewardLayout(SAI2B_REW_FORCE_EXCESS, 0) == 10 && rc.rewardLayout(SAI2B_REW_POS, 0) == -1 && rc.rewardLayout(SAI2B_REW_POS_SQ, 1) == -1,
		  "rows of the terms");
	expect_invalid("rewardLayout of two flags", [&] { rc.rewardLayout(3); });
	Batch out(R * (size_t)B), out2(R * (size_t)B), terms(T * (size_t)B), terms2(T * (size_t)B), tau2(n * (size_t)B);
	std::vector<unsigned char> done(B), done2(B);
	std::vector<double> reward(B), reward2(B);
	expect_invalid("reward of the wrong size", [&] {
		std::vector<double> r(B + 1);
		rc.observeReward(&out, &done, &r, &terms);
	});
	expect_invalid("terms of the wrong size", [&] {
		Batch x((T - 1) * (size_t)B);
		sim.observeReward(&out, &done, &reward, &x);
	});
	expect_invalid("out of the wrong size", [&] {
		Batch x(R * (size_t)B + 1);
		rc.observeReward(&x, &done, &reward, &terms);
	});
	int closed = 0;
	for (int k = 0; k < 6; k++) {
		const Batch tau = rc.tick();
		sim.setJointTorques(tau);
		sim.integrate();
		if (k % 2)	// the members of either class act on the one context
			sim.observeReward(&out, &done, &reward, &terms);
		else
			rc.observeReward(&out, &done, &reward, &terms);
		detail::check(twin, sai2b_tick(twin, tau2.data(), 0));
		detail::check(twin, sai2b_sim_step(twin, tau2.data(), 0, 0.001, 1, 0));
		detail::check(twin, sai2b_observe_reward(twin, out2.data(), done2.data(), reward2.data(), terms2.data(), 0));
		char what[96];
		std::snprintf(what, sizeof(what), "period %d: out, done, reward and terms bit-equal to the C ABI", k);
		check(same(out, out2) && same(done, done2) && same(reward, reward2) && same(terms, terms2), what);
		int c2[2];
		detail::check(twin, sai2b_get_reward_counts(twin, c2));
		const RewardCounts rcnt = rc.rewardCounts();
		check(rcnt.closed == c2[0] && rcnt.replaced == c2[1] && rcnt.replaced == 0, "        counts");
		closed += rcnt.closed;
	}
	check(closed >= B, "every robot closed an episode (the timeout is 4)");
	const EpisodeStats es = sim.episodeStats();
	std::vector<double> ret(B), disc(B), last(B);
	std::vector<int> len(B);
	detail::check(twin, sai2b_get_episode_stats(twin, ret.data(), disc.data(), last.data(), len.data()));
	check(same(es.ret, ret) && same(es.discount, disc) && same(es.last_return, last) && same(es.last_length, len), "episode stats bit-equal to the C ABI");
	bool lengths = true, nonzero = false;
	for (int b = 0; b < B; b++) lengths = lengths && len[b] >= 1 && len[b] <= 4, nonzero = nonzero || last[b] != 0.0;
	check(lengths && nonzero, "last lengths within the timeout, last returns recorded");
	// only the accumulators: nothing wanted
	rc.observeReward(nullptr, nullptr, nullptr, nullptr);
	detail::check(twin, sai2b_observe_reward(twin, nullptr, nullptr, nullptr, nullptr, 0));
	const EpisodeStats es2 = rc.episodeStats();
	detail::check(twin, sai2b_get_episode_stats(twin, ret.data(), disc.data(), last.data(), len.data()));
	check(same(es2.ret, ret) && same(es2.discount, disc) && !same(es2.ret, es.ret), "a call without outputs advances the accumulators");
	rc.clearReward();
	check(rc.rewardRows() == -1 && sim.rewardRows() == -1, "cleared");
	expect_invalid("observeReward after clearReward", [&] { sim.observeReward(&out, &done, &reward, &terms); });
	expect_invalid("rewardCounts after clearReward", [&] { rc.rewardCounts(); });
	expect_invalid("episodeStats after clearReward", [&] { rc.episodeStats(); });
	rc.observe(&out, &done);  // the observation is still there
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
	std::printf("usage: reward_facade_test validate|run\n");
	return 2;
}

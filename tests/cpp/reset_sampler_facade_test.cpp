// The episode-sampler members of the C++ facade (include/Sai2PrimitivesBatched.h: setResetSampler, clearResetSampler,
// resetRobotsSampled, resetSamplerCounts on RobotController and ShardedRobotController) against the C ABI.
//   reset_sampler_facade_test validate   no device: the members exist, the checks ahead of the device throw std::invalid_argument
//   reset_sampler_facade_test run        a sampled reset through the facade, bit-equal to sai2b_reset_robots_sampled on a twin; two
//                                        shards bit-equal to the one context; the exceptions on a live controller
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
	void (T::*set)(const sai2b_reset_sampler_config&, const Batch&) = &T::setResetSampler;
	void (T::*clear)() = &T::clearResetSampler;
	void (T::*reset)(const std::vector<unsigned char>&) = &T::resetRobotsSampled;
	return set && clear && reset;
}

static sai2b_reset_sampler_config configuration() {
	sai2b_reset_sampler_config c;
	sai2b_default_reset_sampler(&c);
	c.seed = 0x1234567890abcdefull, c.max_tries = 6, c.goal_tasks = 3, c.ratio_task = 0, c.min_ratio = 0.05;
	return c;
}

static std::vector<sai2b_task_config> hierarchy() {
	std::vector<sai2b_task_config> tasks(2);
	sai2b_default_motion_force_task(&tasks[0], "m", 6, nullptr, nullptr, -1, nullptr, -1, nullptr);
	sai2b_default_joint_task(&tasks[1], "j", 0, nullptr);
	return tasks;
}

static int validate() {
	if (!has_members<RobotController>() || !has_members<ShardedRobotController>()) return 3;
	const std::vector<sai2b_task_config> tasks = hierarchy();
	const sai2b_reset_sampler_config ok = configuration();
	if (sai2b_sizeof_reset_sampler_config() != (int)sizeof(ok)) return 4;
	const size_t B = 3;
	const int total = detail::checkResetSampler(ok, tasks, SAI2B_DOF, B, {});
	check(total == 4 * 7 + 7 + 7, "42 rows: four joint blocks, a MotionForceTask's seven, a JointTask's seven");
	detail::checkResetSampler(ok, tasks, SAI2B_DOF, B, Batch(42 * B));
	auto with = [&](const std::function<void(sai2b_reset_sampler_config&)>& edit) {
		sai2b_reset_sampler_config c = ok;
		edit(c);
		return c;
	};
	expect_invalid("rows of the wrong size", [&] { detail::checkResetSampler(ok, tasks, SAI2B_DOF, B, Batch(41 * B)); });
	expect_invalid("no tries", [&] { detail::checkResetSampler(with([](auto& c) { c.max_tries = 0; }), tasks, SAI2B_DOF, B, {}); });
	expect_invalid("ratio task is a JointTask", [&] { detail::checkResetSampler(with([](auto& c) { c.ratio_task = 1; }), tasks, SAI2B_DOF, B, {}); });
	expect_invalid("box task out of range", [&] { detail::checkResetSampler(with([](auto& c) { c.box_task = 2; }), tasks, SAI2B_DOF, B, {}); });
	expect_invalid("goal of a task that is not there", [&] { detail::checkResetSampler(with([](auto& c) { c.goal_tasks = 4; }), tasks, SAI2B_DOF, B, {}); });
	expect_invalid("absolute position of a JointTask", [&] { detail::checkResetSampler(with([](auto& c) { c.absolute_position = 2; }), tasks, SAI2B_DOF, B, {}); });
	expect_invalid("ratio above one", [&] { detail::checkResetSampler(with([](auto& c) { c.min_ratio = 2.0; }), tasks, SAI2B_DOF, B, {}); });
	expect_invalid("mask of the wrong size", [&] { detail::checkResetArguments(7, B, std::vector<unsigned char>(B + 1), {}, {}, "resetRobotsSampled"); });
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
	Batch q(n * (size_t)B), dq(n * (size_t)B, 0.0);
	for (int b = 0; b < B; b++)
		for (int i = 0; i < n; i++) q[i * (size_t)B + b] = q0[i] + 0.3 * std::sin(0.37 * b + i);
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
		r.jt = std::make_shared<JointTask>(r.robot, "jt");
		std::vector<std::shared_ptr<TemplateTask>> tasks = {r.mft, r.jt};
		r.rc = std::make_unique<RobotController>(r.robot, tasks);
		return r;
	};
	Rig a = build(), t = build();
	RobotController& rc = *a.rc;
	sai2b_ctx* twin = t.rc->ctx();
	const sai2b_reset_sampler_config cfg = configuration();
	std::vector<unsigned char> mask(B);
	for (int b = 0; b < B; b++) mask[b] = b % 3 != 1;
	expect_invalid("resetRobotsSampled before setResetSampler", [&] { rc.resetRobotsSampled(mask); });
	expect_invalid("resetSamplerCounts before setResetSampler", [&] { rc.resetSamplerCounts(); });
	// rows: the defaults with a goal box and a velocity
	int total = 0, first = 0, rows_n = 0;
	std::vector<sai2b_task_config> cfgs = {a.mft->config(), a.jt->config()};
	detail::check(nullptr, sai2b_reset_sampler_config_layout(&cfg, cfgs.data(), 2, n, 4, 0, &first, &rows_n, &total));
	rc.setResetSampler(cfg);
	Batch rows(total * (size_t)B);
	sai2b_reset_sampler_config back;
	detail::check(rc.ctx(), sai2b_get_reset_sampler(rc.ctx(), &back, rows.data()));
	check(back.seed == cfg.seed && back.max_tries == 6 && rows_n == 7 && total == 42, "the configuration and the default rows come back");
	for (int b = 0; b < B; b++) {
		for (int i = 0; i < n; i++) rows[(2 * n + i) * (size_t)B + b] = 0.05 * (i + 1);
		for (int k = 0; k < 3; k++) rows[(first + k) * (size_t)B + b] = -0.05, rows[(first + 3 + k) * (size_t)B + b] = 0.02 * (k + 1);
		rows[(first + 6) * (size_t)B + b] = 0.4;
	}
	expect_invalid("rows of the wrong size", [&] { rc.setResetSampler(cfg, Batch(rows.size() - 1)); });
	expect_invalid("mask of the wrong size", [&] { rc.resetRobotsSampled(std::vector<unsigned char>(B - 1)); });
	rc.setResetSampler(cfg, rows);
	detail::check(twin, sai2b_set_reset_sampler(twin, &cfg, rows.data(), 0));
	auto state = [&](sai2b_ctx* c) {
		Batch s(2 * n * (size_t)B + 12 * (size_t)B + n * (size_t)B);
		detail::check(c, sai2b_get_state(c, s.data(), s.data() + n * (size_t)B));
		double* g = s.data() + 2 * n * (size_t)B;
		detail::check(c, sai2b_get_mft_goals(c, 0, g, g + 3 * (size_t)B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
		detail::check(c, sai2b_get_jt_goals(c, 1, g + 12 * (size_t)B, nullptr, nullptr));
		return s;
	};
	for (int k = 0; k < 2; k++) {
		rc.resetRobotsSampled(mask);
		detail::check(twin, sai2b_reset_robots_sampled(twin, mask.data(), 0));
		check(same(state(rc.ctx()), state(twin)), "state and goals bit-equal to the C ABI");
		int c2[3];
		detail::check(twin, sai2b_get_reset_sampler_counts(twin, c2));
		const ResetSamplerCounts c = rc.resetSamplerCounts();
		check(c.reset == c2[0] && c.rejected == c2[1] && c.exhausted == c2[2] && c.reset == 87 && c.rejected > 0, "counts");
	}
	const Batch one = state(rc.ctx());
	// two shards on the one device, driven alike: the robots draw what they draw in the one context
	{
		ShardedRobotController sh(model, cfgs, B, {0, 0});
		sh.setState(q, dq);
		sh.reinitializeTasks();
		sh.setResetSampler(cfg, rows);
		for (int k = 0; k < 2; k++) sh.resetRobotsSampled(mask);
		Batch got(one.size());
		for (int s = 0; s < sh.shards(); s++) {
			const auto [lo, hi] = sh.shardBounds(s);
			const size_t Bs = hi - lo;
			Batch part(2 * n * Bs + 12 * Bs + n * Bs);
			sai2b_ctx* c = sh.ctx(s);
			detail::check(c, sai2b_get_state(c, part.data(), part.data() + n * Bs));
			double* g = part.data() + 2 * n * Bs;
			detail::check(c, sai2b_get_mft_goals(c, 0, g, g + 3 * Bs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
			detail::check(c, sai2b_get_jt_goals(c, 1, g + 12 * Bs, nullptr, nullptr));
			for (size_t r = 0; r < (size_t)(2 * n + 12 + n); r++)
				for (size_t b = 0; b < Bs; b++) got[r * (size_t)B + lo + b] = part[r * Bs + b];
		}
		bool equal = true;
		for (size_t r = 0; r < (size_t)(2 * n + 12 + n); r++)
			for (int b = 0; b < B; b++)
				if (mask[b] && std::memcmp(&got[r * (size_t)B + b], &one[r * (size_t)B + b], sizeof(double))) equal = false;
		check(equal, "two shards bit-equal to the one context for the selected robots");
		const ResetSamplerCounts c = sh.resetSamplerCounts();
		check(c.reset == 87, "counts summed over the shards");
		expect_invalid("sharded mask of the wrong size", [&] { sh.resetRobotsSampled(std::vector<unsigned char>(B + 2)); });
		sh.clearResetSampler();
		expect_invalid("sharded reset after clear", [&] { sh.resetRobotsSampled(mask); });
	}
	rc.clearResetSampler();
	expect_invalid("resetRobotsSampled after clearResetSampler", [&] { rc.resetRobotsSampled(mask); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

int main(int argc, char** argv) {
	if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
	if (argc == 2 && !std::strcmp(argv[1], "run")) return run();
	std::fprintf(stderr, "usage: reset_sampler_facade_test validate | run\n");
	return 2;
}

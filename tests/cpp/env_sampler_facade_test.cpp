// The environment-sampler members of the C++ facade (include/Sai2PrimitivesBatched.h: setEnvSampler, clearEnvSampler,
// randomizeRobots, envSamplerCounts on RobotController and ShardedRobotController) against the C ABI.
//   env_sampler_facade_test validate   no device: the members exist, the checks ahead of the device throw std::invalid_argument
//   env_sampler_facade_test run        three calls through the facade, bit-equal to sai2b_randomize_robots on a twin; two shards
//                                      bit-equal to the one context; the exceptions on a live controller
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
	void (T::*set)(const sai2b_env_sampler_config&) = &T::setEnvSampler;
	void (T::*clear)() = &T::clearEnvSampler;
	void (T::*draw)(const std::vector<unsigned char>&, unsigned) = &T::randomizeRobots;
	return set && clear && draw;
}

// contact and push: the two groups whose features the test sets through the C ABI
static sai2b_env_sampler_config configuration() {
	sai2b_env_sampler_config c;
	sai2b_default_env_sampler(&c);
	c.seed = 0x1234567890abcdefull, c.groups = SAI2B_ENV_CONTACT | SAI2B_ENV_PUSH;
	c.contact_height.lower = -0.01, c.contact_height.upper = 0.02, c.contact_tilt_max = 0.3;
	c.contact_stiffness_scale.lower = 0.5, c.contact_stiffness_scale.upper = 2.0, c.contact_stiffness_scale.log_uniform = 1;
	c.push_force.lower = 1.0, c.push_force.upper = 5.0, c.push_steps_lower = 2, c.push_steps_upper = 9;
	return c;
}

static int validate() {
	if (!has_members<RobotController>() || !has_members<ShardedRobotController>()) return 3;
	const sai2b_env_sampler_config ok = configuration();
	if (sai2b_sizeof_env_sampler_config() != (int)sizeof(ok)) return 4;
	detail::checkEnvSampler(ok, SAI2B_DOF);
	int first = 0, rows = 0, total = 0;
	check(sai2b_env_sampler_config_layout(&ok, SAI2B_DOF, SAI2B_ENV_PUSH, &first, &rows, &total) == SAI2B_OK && first == 8 && rows == 9 && total == 17,
		  "17 sample rows: the contact's eight, the push's nine");
	auto with = [&](const std::function<void(sai2b_env_sampler_config&)>& edit) {
		sai2b_env_sampler_config c = ok;
		edit(c);
		return c;
	};
	expect_invalid("a group that is none", [&] { detail::checkEnvSampler(with([](auto& c) { c.groups = 64; }), SAI2B_DOF); });
	expect_invalid("the controller's payload alone", [&] { detail::checkEnvSampler(with([](auto& c) { c.payload_target = SAI2B_PAYLOAD_CONTROLLER; }), SAI2B_DOF); });
	expect_invalid("a range upside down", [&] { detail::checkEnvSampler(with([](auto& c) { c.push_force.upper = 0.5; }), SAI2B_DOF); });
	expect_invalid("a log-uniform range from zero", [&] { detail::checkEnvSampler(with([](auto& c) { c.contact_stiffness_scale.lower = 0.0; }), SAI2B_DOF); });
	expect_invalid("a lag scale of zero", [&] { detail::checkEnvSampler(with([](auto& c) { c.lag_scale.lower = 0.0; }), SAI2B_DOF); });
	expect_invalid("a tilt beyond pi", [&] { detail::checkEnvSampler(with([](auto& c) { c.contact_tilt_max = 3.2; }), SAI2B_DOF); });
	expect_invalid("a delay beyond the deepest history", [&] { detail::checkEnvSampler(with([](auto& c) { c.delay_upper = 9; }), SAI2B_DOF); });
	expect_invalid("mask of the wrong size", [&] { detail::checkResetArguments(7, 3, std::vector<unsigned char>(4), {}, {}, "randomizeRobots"); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
	return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

static int run() {
	const int B = 130, n = 7, S = 17;
	sai2b_robot_model model;
	detail::check(nullptr, sai2b_panda_model(&model));
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5}, frame[3] = {0.0, 0.0, 0.1};
	Batch q(n * (size_t)B), dq(n * (size_t)B, 0.0);
	for (int b = 0; b < B; b++)
		for (int i = 0; i < n; i++) q[i * (size_t)B + b] = q0[i] + 0.3 * std::sin(0.37 * b + i);
	// per-robot planes and pushes for the whole batch
	Batch point(3 * (size_t)B), normal(3 * (size_t)B), stiff(B), damp(B), mu(B), force(3 * (size_t)B, 0.0), steps(B, 0.0);
	for (int b = 0; b < B; b++) {
		const double a = 0.1 * std::sin(0.9 * b), c = 0.1 * std::cos(1.3 * b), z = std::sqrt(1.0 - a * a - c * c);
		normal[b] = a, normal[B + b] = c, normal[2 * (size_t)B + b] = z;
		point[b] = 0.4, point[B + b] = 0.01 * b, point[2 * (size_t)B + b] = 0.2 + 0.001 * b;
		stiff[b] = 1000.0 + 10.0 * b, damp[b] = 0.1, mu[b] = 0.3 + 0.001 * b;
	}
	struct Rig {
		std::shared_ptr<BatchedRobotModel> robot;
		std::shared_ptr<MotionForceTask> mft;
		std::shared_ptr<JointTask> jt;
		std::unique_ptr<RobotController> rc;
	};
	// the features of the two groups, through the C ABI, for the robots [lo, lo + Bs) of the batch
	auto features = [&](sai2b_ctx* c, size_t lo, size_t Bs) {
		auto part = [&](const Batch& v, int rows) {
			Batch out(rows * Bs);
			for (int r = 0; r < rows; r++)
				for (size_t b = 0; b < Bs; b++) out[r * Bs + b] = v[r * (size_t)B + lo + b];
			return out;
		};
		sai2b_contact_config cc;
		detail::check(c, sai2b_default_contact(&cc, 6, 1, nullptr));
		const Batch p = part(point, 3), nn = part(normal, 3), k = part(stiff, 1), d = part(damp, 1), m = part(mu, 1);
		detail::check(c, sai2b_set_contact(c, &cc, p.data(), nn.data(), k.data(), d.data(), m.data(), 0));
		sai2b_external_wrench_config wc;
		detail::check(c, sai2b_default_external_wrench(&wc, 6));
		const Batch f = part(force, 3), st = part(steps, 1);
		detail::check(c, sai2b_set_external_wrench(c, &wc, f.data(), nullptr, st.data(), 0));
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
	const sai2b_env_sampler_config cfg = configuration();
	std::vector<unsigned char> mask(B);
	for (int b = 0; b < B; b++) mask[b] = b % 3 != 1;
	expect_invalid("randomizeRobots before setEnvSampler", [&] { rc.randomizeRobots(mask); });
	expect_invalid("envSamplerCounts before setEnvSampler", [&] { rc.envSamplerCounts(); });
	expect_invalid("setEnvSampler before the features are set", [&] { rc.setEnvSampler(cfg); });
	features(rc.ctx(), 0, B), features(twin, 0, B);
	rc.setEnvSampler(cfg);
	detail::check(twin, sai2b_set_env_sampler(twin, &cfg));
	sai2b_env_sampler_config back;
	detail::check(rc.ctx(), sai2b_get_env_sampler(rc.ctx(), &back));
	check(back.seed == cfg.seed && back.groups == cfg.groups && back.push_steps_upper == 9, "the configuration comes back");
	// contact rows 9, wrench rows 7, sample rows S, the counter as doubles
	auto state = [&](sai2b_ctx* c, size_t Bs) {
		Batch s((9 + 7 + S + 1) * Bs);
		std::vector<int> counter(Bs);
		detail::check(c, sai2b_get_contact(c, nullptr, s.data()));
		detail::check(c, sai2b_get_external_wrench(c, nullptr, s.data() + 9 * Bs));
		detail::check(c, sai2b_get_env_sampler_state(c, counter.data(), s.data() + 16 * Bs));
		for (size_t b = 0; b < Bs; b++) s[(16 + S) * Bs + b] = counter[b];
		return s;
	};
	expect_invalid("mask of the wrong size", [&] { rc.randomizeRobots(std::vector<unsigned char>(B - 1)); });
	expect_invalid("a group that was not configured", [&] { rc.randomizeRobots(mask, SAI2B_ENV_HARDWARE); });
	const unsigned groups[3] = {0, SAI2B_ENV_PUSH, SAI2B_ENV_CONTACT};
	for (int k = 0; k < 3; k++) {
		rc.randomizeRobots(mask, groups[k]);
		detail::check(twin, sai2b_randomize_robots(twin, mask.data(), groups[k], 0));
		check(same(state(rc.ctx(), B), state(twin, B)), "rows, sample rows and counters bit-equal to the C ABI");
		int c2[2];
		detail::check(twin, sai2b_get_env_sampler_counts(twin, c2));
		const EnvSamplerCounts c = rc.envSamplerCounts();
		check(c.drawn == c2[0] && c.lag_clipped == c2[1] && c.drawn == 87 && c.lag_clipped == 0, "counts");
	}
	const Batch one = state(rc.ctx(), B);
	check(one[(16 + S) * (size_t)B] == 3.0 && one[(16 + S) * (size_t)B + 1] == 0.0 && one[9 * (size_t)B + 6 * (size_t)B] >= 2.0, "three draws of robot 0, none of robot 1");
	// two shards on the one device, driven alike: the robots draw what they draw in the one context
	{
		std::vector<sai2b_task_config> cfgs = {a.mft->config(), a.jt->config()};
		ShardedRobotController sh(model, cfgs, B, {0, 0});
		sh.setState(q, dq);
		sh.reinitializeTasks();
		expect_invalid("sharded setEnvSampler before the features are set", [&] { sh.setEnvSampler(cfg); });
		for (int s = 0; s < sh.shards(); s++) {
			const auto [lo, hi] = sh.shardBounds(s);
			features(sh.ctx(s), lo, hi - lo);
		}
		sh.setEnvSampler(cfg);
		for (int k = 0; k < 3; k++) sh.randomizeRobots(mask, groups[k]);
		Batch got(one.size());
		for (int s = 0; s < sh.shards(); s++) {
			const auto [lo, hi] = sh.shardBounds(s);
			const size_t Bs = hi - lo;
			const Batch part = state(sh.ctx(s), Bs);
			for (size_t r = 0; r < (size_t)(17 + S); r++)
				for (size_t b = 0; b < Bs; b++) got[r * (size_t)B + lo + b] = part[r * Bs + b];
		}
		check(same(got, one), "two shards bit-equal to the one context");
		const EnvSamplerCounts c = sh.envSamplerCounts();
		check(c.drawn == 87 && c.lag_clipped == 0, "counts summed over the shards");
		expect_invalid("sharded mask of the wrong size", [&] { sh.randomizeRobots(std::vector<unsigned char>(B + 2)); });
		sh.clearEnvSampler();
		expect_invalid("sharded draw after clear", [&] { sh.randomizeRobots(mask); });
	}
	detail::check(rc.ctx(), sai2b_clear_contact(rc.ctx()));
	expect_invalid("a feature cleared since", [&] { rc.randomizeRobots(mask); });
	rc.randomizeRobots(mask, SAI2B_ENV_PUSH);
	check(rc.envSamplerCounts().drawn == 87, "the push alone still draws");
	rc.clearEnvSampler();
	expect_invalid("randomizeRobots after clearEnvSampler", [&] { rc.randomizeRobots(mask); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

int main(int argc, char** argv) {
	if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
	if (argc == 2 && !std::strcmp(argv[1], "run")) return run();
	std::fprintf(stderr, "usage: env_sampler_facade_test validate | run\n");
	return 2;
}

// The inverse-kinematics members of the C++ facade (include/Sai2PrimitivesBatched.h: setInverseKinematics, clearInverseKinematics,
// getInverseKinematics, solveInverseKinematics, getInverseKinematicsCounts on RobotController and BatchedSimulation, mirrored on
// ShardedRobotController).
// `validate <urdf>` needs no device: the members by signature, the struct's size, and the std::invalid_argument conditions that
// are judged ahead of the device, each with the validator's message. `run <urdf> <goal.f64> <seed.f64> <out.f64>`: B Pandas
// (B from the size of seed.f64, [7][B]) with a MotionForceTask at the end-effector body, one solve of the goals [12][B] through
// RobotController, the same through BatchedSimulation under a mask, a ShardedRobotController of two shards bit-equal to the one
// context, the counts, the exceptions of the members themselves;
// out.f64 receives q [7][B], status [5][B] and the flags as doubles [B] for tests/test_cpp_ik_facade.py to hold to the reference.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <type_traits>

#include "Sai2PrimitivesBatched.h"

using namespace Sai2Primitives;

static int failures = 0;
static void check(bool ok, const char* name) {
	std::printf("%s %s\n", ok ? "ok" : "FAILED", name);
	if (!ok) failures++;
}
static void expect_invalid(const char* what, const char* word, const std::function<void()>& f) {
	try {
		f();
	} catch (const std::invalid_argument& e) {
		const bool has = std::strstr(e.what(), word) != nullptr;
		std::printf("%s %s: %s\n", has ? "ok  " : "FAILED", what, e.what());
		if (!has) failures++;
		return;
	} catch (const std::exception& e) {
		std::printf("FAILED %s: threw %s\n", what, e.what());
		failures++;
		return;
	}
	std::printf("FAILED %s: did not throw\n", what);
	failures++;
}

static bool read_all(const char* path, Batch& v) {
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	std::fseek(f, 0, SEEK_END);
	const long bytes = std::ftell(f);
	std::fseek(f, 0, SEEK_SET);
	v.resize(bytes > 0 ? (size_t)bytes / sizeof(double) : 0);
	const size_t got = v.empty() ? 0 : std::fread(v.data(), sizeof(double), v.size(), f);
	std::fclose(f);
	return got == v.size();
}

static int validate(const char* urdf) {
	using M = detail::IkMembers;
	static_assert(std::is_base_of<M, RobotController>::value && std::is_base_of<M, BatchedSimulation>::value, "both classes have the members");
	static_assert(std::is_same<decltype(&M::setInverseKinematics), void (M::*)(const sai2b_ik_config&)>::value, "setInverseKinematics");
	static_assert(std::is_same<decltype(&M::clearInverseKinematics), void (M::*)()>::value, "clearInverseKinematics");
	static_assert(std::is_same<decltype(&M::solveInverseKinematics), IkResult (M::*)(const Batch&, const Batch&, const std::vector<unsigned char>&)>::value,
				  "solveInverseKinematics");
	static_assert(std::is_same<decltype(&M::getInverseKinematicsCounts), IkCounts (M::*)() const>::value, "getInverseKinematicsCounts");
	using S = ShardedRobotController;
	static_assert(std::is_same<decltype(&S::setInverseKinematics), void (S::*)(const sai2b_ik_config&)>::value, "sharded setInverseKinematics");
	static_assert(std::is_same<decltype(&S::clearInverseKinematics), void (S::*)()>::value, "sharded clearInverseKinematics");
	static_assert(std::is_same<decltype(&S::solveInverseKinematics), IkResult (S::*)(const Batch&, const Batch&, const std::vector<unsigned char>&)>::value,
				  "sharded solveInverseKinematics");
	static_assert(std::is_same<decltype(&S::getInverseKinematicsCounts), IkCounts (S::*)()>::value, "sharded getInverseKinematicsCounts");
	check(sai2b_sizeof_ik_config() == (int)sizeof(sai2b_ik_config), "size of the configuration");
	BatchedRobotModel robot(urdf, 4);
	sai2b_ik_config cfg;
	check(sai2b_default_ik(&cfg) == SAI2B_OK && cfg.axes == 63 && cfg.max_iterations == 40 && cfg.restarts == 0 && cfg.mu0 == 1e-2, "the defaults");
	detail::checkIkConfig(cfg, 7, &robot.model(), "x");
	auto changed = [&](const std::function<void(sai2b_ik_config&)>& f) {
		sai2b_ik_config c = cfg;
		f(c);
		return c;
	};
	expect_invalid("no axis", "axes", [&] { detail::checkIkConfig(changed([](sai2b_ik_config& c) { c.axes = 0; }), 7, nullptr, "setInverseKinematics"); });
	expect_invalid("201 iterations", "max_iterations", [&] { detail::checkIkConfig(changed([](sai2b_ik_config& c) { c.max_iterations = 201; }), 7, nullptr, "x"); });
	expect_invalid("mu_down 1", "mu_down", [&] { detail::checkIkConfig(changed([](sai2b_ik_config& c) { c.mu_down = 1.0; }), 7, nullptr, "x"); });
	expect_invalid("a step that is not finite", "step_max", [&] { detail::checkIkConfig(changed([](sai2b_ik_config& c) { c.step_max = NAN; }), 7, nullptr, "x"); });
	expect_invalid("restarts without limits", "restarts need use_limits",
				   [&] { detail::checkIkConfig(changed([](sai2b_ik_config& c) { c.restarts = 2, c.use_limits = 0; }), 7, &robot.model(), "x"); });
	expect_invalid("a margin that leaves no interval", "interval",
				   [&] { detail::checkIkConfig(changed([](sai2b_ik_config& c) { c.limit_margin = 3.0; }), 7, &robot.model(), "x"); });
	expect_invalid("a robot size without a build", "", [&] { detail::checkIkConfig(cfg, 5, nullptr, "x"); });
	expect_invalid("goal rows of another shape", "goal_rows", [&] { detail::checkIkRows(cfg, 7, 4, Batch(11 * 4), Batch(7 * 4), {}); });
	expect_invalid("seed rows of another shape", "seed_rows", [&] { detail::checkIkRows(cfg, 7, 4, Batch(12 * 4), Batch(6 * 4), {}); });
	expect_invalid("a short mask", "mask", [&] { detail::checkIkRows(cfg, 7, 4, Batch(12 * 4), Batch(7 * 4), std::vector<unsigned char>(3)); });
	detail::checkIkRows(cfg, 7, 4, Batch(12 * 4), Batch(7 * 4), std::vector<unsigned char>(4));
	detail::checkIkRows(changed([](sai2b_ik_config& c) { c.rest_weight = 0.1, c.seed_source = SAI2B_IK_STATE; }), 7, 4, Batch(19 * 4), {}, {});
	const IkResult empty = detail::emptyIkResult(7, 4);
	check(empty.q.size() == 28 && empty.status.size() == 20 && empty.flags.size() == 4 && std::isnan(empty.q[0]) && empty.flags[3] == 0, "an empty result");
	check(sai2b_set_ik(nullptr, &cfg) == SAI2B_INVALID_ARGUMENT && sai2b_solve_ik(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == SAI2B_INVALID_ARGUMENT,
		  "the C calls reject a NULL context");
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

static int run(const char* urdf, const char* goal_path, const char* seed_path, const char* out_path) {
	const int n = 7;
	Batch goal, seed;
	if (!read_all(goal_path, goal) || !read_all(seed_path, seed) || seed.empty() || seed.size() % n || goal.size() != 12 * (seed.size() / n)) return 2;
	const int B = (int)(seed.size() / n);
	const size_t sB = (size_t)B;
	auto robot = std::make_shared<BatchedRobotModel>(urdf, B, 0);
	robot->setQ(seed);
	robot->setDq(Batch(n * sB, 0.0));
	robot->updateModel();
	const double fp[3] = {0.0, 0.0, 0.15};
	auto mft = std::make_shared<MotionForceTask>(robot, "end-effector", fp);
	auto jt = std::make_shared<JointTask>(robot, "jt");
	std::vector<std::shared_ptr<TemplateTask>> tasks = {mft, jt};
	RobotController rc(robot, tasks);
	BatchedSimulation sim(rc, 0.001, 1);
	expect_invalid("a solve before the configuration", "no inverse kinematics", [&] { rc.solveInverseKinematics(goal, seed); });
	sai2b_ik_config cfg;
	sai2b_default_ik(&cfg);
	sai2b_ik_config bad = cfg;
	bad.task = 1;
	expect_invalid("the JointTask", "MotionForceTask", [&] { rc.setInverseKinematics(bad); });
	bad = cfg, bad.tol_pos = -1.0;
	expect_invalid("a negative tolerance", "tol_pos", [&] { rc.setInverseKinematics(bad); });
	expect_invalid("still no configuration", "no inverse kinematics", [&] { rc.getInverseKinematics(); });
	rc.setInverseKinematics(cfg);
	check(sim.getInverseKinematics().max_iterations == 40, "the simulation's members act on the controller's context");
	const IkResult r = rc.solveInverseKinematics(goal, seed);
	const IkCounts c = rc.getInverseKinematicsCounts();
	int converged = 0;
	for (int b = 0; b < B; b++) converged += (r.flags[b] & SAI2B_IK_CONVERGED) != 0;
	check(c.selected == B && c.converged == converged && c.exhausted == B - converged && c.nonfinite == 0, "counts");
	// under a mask, through the simulation: the selected robots bit for bit, the others NaN and flag 0
	std::vector<unsigned char> mask(B, 0);
	for (int b = 0; b < B; b += 3) mask[b] = 1;
	const IkResult m = sim.solveInverseKinematics(goal, seed, mask);
	bool same = true, untouched = true;
	for (int b = 0; b < B; b++)
		for (int i = 0; i < n; i++) {
			if (mask[b])
				same = same && m.q[i * sB + b] == r.q[i * sB + b] && m.flags[b] == r.flags[b];
			else
				untouched = untouched && std::isnan(m.q[i * sB + b]) && m.flags[b] == 0;
		}
	check(same && untouched && sim.getInverseKinematicsCounts().selected == (B + 2) / 3, "a masked solve");
	expect_invalid("goal rows of another shape", "goal_rows", [&] { rc.solveInverseKinematics(Batch(11 * sB), seed); });
	expect_invalid("no seed rows", "seed_rows", [&] { rc.solveInverseKinematics(goal); });
	// the seed from the state: the robot was put at the seeds above
	sai2b_ik_config from_state = cfg;
	from_state.seed_source = SAI2B_IK_STATE;
	rc.setInverseKinematics(from_state);
	const IkResult s = rc.solveInverseKinematics(goal);
	check(s.q == r.q && s.flags == r.flags, "the seed from the state");
	// two shards on one device against the single context, bit for bit: restarts, so that first_robot matters; a mask; the counts
	{
		sai2b_ik_config far = cfg;
		far.max_iterations = 6, far.restarts = 2, far.seed = 11, far.first_robot = 1000;
		rc.setInverseKinematics(far);
		const IkResult one = rc.solveInverseKinematics(goal, seed, mask);
		const IkCounts c1 = rc.getInverseKinematicsCounts();
		ShardedRobotController sh(robot->model(), {mft->config(), jt->config()}, B, {0, 0});
		expect_invalid("a sharded solve before the configuration", "no inverse kinematics", [&] { sh.solveInverseKinematics(goal, seed); });
		sh.setInverseKinematics(far);
		const IkResult two = sh.solveInverseKinematics(goal, seed, mask);
		const IkCounts c2 = sh.getInverseKinematicsCounts();
		bool equal = two.flags == one.flags && two.q.size() == one.q.size() && two.status.size() == one.status.size();
		for (size_t i = 0; equal && i < one.q.size(); i++) equal = std::memcmp(&two.q[i], &one.q[i], sizeof(double)) == 0;
		for (size_t i = 0; equal && i < one.status.size(); i++) equal = std::memcmp(&two.status[i], &one.status[i], sizeof(double)) == 0;
		int restarted = 0;
		for (int b = 0; b < B; b++) restarted += mask[b] && one.status[2 * sB + b] > far.max_iterations;  // more iterations than one start has
		if (!equal || restarted == 0) {
			int fq = 0, ff = 0, fs = 0, first = -1;
			for (int b = 0; b < B; b++) {
				bool bad = two.flags[b] != one.flags[b];
				ff += bad;
				for (int i = 0; i < n; i++) {
					const bool d = std::memcmp(&two.q[i * sB + b], &one.q[i * sB + b], sizeof(double)) != 0;
					fq += d, bad = bad || d;
				}
				for (int i = 0; i < SAI2B_IK_STATUS_ROWS; i++) fs += std::memcmp(&two.status[i * sB + b], &one.status[i * sB + b], sizeof(double)) != 0;
				if (bad && first < 0) first = b;
			}
			std::printf("   differing: q %d, status %d, flags %d entries; first robot %d (mask %d, start %g vs %g, flags %d vs %d); restarted %d\n", fq, fs, ff, first,
						first >= 0 ? mask[first] : -1, first >= 0 ? one.status[3 * sB + first] : 0.0, first >= 0 ? two.status[3 * sB + first] : 0.0,
						first >= 0 ? one.flags[first] : 0, first >= 0 ? two.flags[first] : 0, restarted);
		}
		check(equal && restarted > 0, "two shards equal one context bit for bit, restarts and mask included");
		check(c1.selected == c2.selected && c1.converged == c2.converged && c1.exhausted == c2.exhausted && c2.selected == (B + 2) / 3, "sharded counts");
		sh.clearInverseKinematics();
		expect_invalid("a sharded solve after clearInverseKinematics", "no inverse kinematics", [&] { sh.solveInverseKinematics(goal, seed); });
	}
	rc.clearInverseKinematics();
	expect_invalid("a solve after clearInverseKinematics", "no inverse kinematics", [&] { sim.solveInverseKinematics(goal, seed); });
	Batch out;
	out.insert(out.end(), r.q.begin(), r.q.end());
	out.insert(out.end(), r.status.begin(), r.status.end());
	for (int b = 0; b < B; b++) out.push_back((double)r.flags[b]);
	FILE* f = std::fopen(out_path, "wb");
	if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
	std::fclose(f);
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

int main(int argc, char** argv) {
	if (argc == 3 && !std::strcmp(argv[1], "validate")) return validate(argv[2]);
	if (argc == 6 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3], argv[4], argv[5]);
	std::fprintf(stderr, "usage: ik_facade_test validate <panda urdf> | run <panda urdf> <goal> <seed> <out>\n");
	return 2;
}

// The whole-arm contact members of the C++ facade (include/Sai2PrimitivesBatched.h: setBodyContact, clearBodyContact,
// getBodyContact, getBodyContactState, robotsTouching on BatchedSimulation; setBodyContact, clearBodyContact, getBodyContactState
// on ShardedRobotController).
// `validate` needs no device: the members by signature, the struct's size, and the std::invalid_argument conditions that are
// judged ahead of the device. `run <urdf> <in> <out>`: the inputs tests/test_cpp_body_contact_facade.py wrote (doubles: B, S, P,
// O, categories, v_eps, periods, substeps; q, dq, tau [7][B]; links [S], centres [S][3], radii [S]; environment rows
// [6 P + 4 O][B]; rows [3][B]) through `periods` periods of integrate(); after every period q, dq [7][B], the status [16][B] and
// the four counts go to <out>, where the Python mirror is held against them. Then the members' own exceptions, which leave the
// contact as it was, clearBodyContact and clearCollision; then the ShardedRobotController's members on two shards with explicit
// pairs and every category, status and counts of two periods appended to <out>.
#include <cmath>
#include <cstdlib>
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
static void expect_invalid(const char* what, const std::function<void()>& f) {
	try {
		f();
	} catch (const std::invalid_argument& e) {
		std::printf("ok   %s: %s\n", what, e.what());
		return;
	} catch (const std::exception& e) {
		std::printf("FAILED %s: threw %s\n", what, e.what());
		failures++;
		return;
	}
	std::printf("FAILED %s: did not throw\n", what);
	failures++;
}

static int validate() {
	using M = detail::CollisionMembers;
	static_assert(std::is_base_of<M, BatchedSimulation>::value, "BatchedSimulation has the members");
	static_assert(std::is_same<decltype(&M::setBodyContact), void (M::*)(const Batch&, const Batch&, const Batch&, int, double)>::value, "setBodyContact");
	static_assert(std::is_same<decltype(&M::clearBodyContact), void (M::*)()>::value, "clearBodyContact");
	static_assert(std::is_same<decltype(&M::getBodyContact), Batch (M::*)(int*) const>::value, "getBodyContact");
	static_assert(std::is_same<decltype(&M::getBodyContactState), BodyContactState (M::*)() const>::value, "getBodyContactState");
	static_assert(std::is_same<decltype(&M::robotsTouching), int (M::*)() const>::value, "robotsTouching");
	using S = ShardedRobotController;
	static_assert(std::is_same<decltype(&S::setBodyContact), void (S::*)(const Batch&, int, double)>::value, "sharded setBodyContact");
	static_assert(std::is_same<decltype(&S::clearBodyContact), void (S::*)()>::value, "sharded clearBodyContact");
	static_assert(std::is_same<decltype(&S::getBodyContactState), BodyContactState (S::*)()>::value, "sharded getBodyContactState");
	check(true, "members compile");
	check(sai2b_sizeof_body_contact_config() == (int)sizeof(sai2b_body_contact_config), "size of the configuration");
	check(detail::BODY_CONTACT_ALL == 7, "every category");
	const Batch k(4, 2e4), three(12, 0.5);
	check(detail::bodyContactRows(4, k, {}, {}) == Batch({2e4, 2e4, 2e4, 2e4, 0, 0, 0, 0, 0, 0, 0, 0}), "damping and friction default to 0");
	const sai2b_body_contact_config cfg = detail::bodyContactConfig(7, 4, three, 5, 2e-3);
	check(cfg.categories == 5 && cfg.v_eps == 2e-3, "the configuration");
	expect_invalid("stiffness of another length", [&] { detail::bodyContactRows(4, Batch(3, 1.0), {}, {}); });
	expect_invalid("damping of another length", [&] { detail::bodyContactRows(4, k, Batch(5, 0.0), {}); });
	expect_invalid("rows of another shape", [&] { detail::bodyContactConfig(7, 4, Batch(11, 0.0), 7, 1e-3); });
	expect_invalid("no category", [&] { detail::bodyContactConfig(7, 4, three, 0, 1e-3); });
	expect_invalid("an unknown category", [&] { detail::bodyContactConfig(7, 4, three, 8, 1e-3); });
	expect_invalid("v_eps = 0", [&] { detail::bodyContactConfig(7, 4, three, 7, 0.0); });
	expect_invalid("a NaN v_eps", [&] { detail::bodyContactConfig(7, 4, three, 7, NAN); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

static bool read_doubles(const char* path, Batch& v) {
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

static int run(const char* urdf, const char* in_path, const char* out_path) {
	Batch in;
	if (!read_doubles(in_path, in) || in.size() < 8) return 2;
	const int B = (int)in[0], S = (int)in[1], P = (int)in[2], O = (int)in[3], categories = (int)in[4], periods = (int)in[6], substeps = (int)in[7], n = 7;
	const double v_eps = in[5];
	const size_t sB = (size_t)B, env_rows = (size_t)(6 * P + 4 * O);
	if (in.size() != 8 + 3 * n * sB + 5 * (size_t)S + env_rows * sB + 3 * sB) return 2;
	const double* p = in.data() + 8;
	auto take = [&](size_t count) {
		Batch v(p, p + count);
		p += count;
		return v;
	};
	const Batch q = take(n * sB), dq = take(n * sB), tau = take(n * sB), links_d = take(S), centres = take(3 * (size_t)S), radii = take(S);
	const Batch env = take(env_rows * sB), rows = take(3 * sB);
	std::vector<int> links(S);
	for (int k = 0; k < S; k++) links[k] = (int)links_d[k];
	auto robot = std::make_shared<BatchedRobotModel>(urdf, B, 0);
	robot->setQ(q);
	robot->setDq(dq);
	robot->updateModel();
	const double fp[3] = {0.0, 0.0, 0.15};
	auto mft = std::make_shared<MotionForceTask>(robot, "end-effector", fp);
	auto jt = std::make_shared<JointTask>(robot, "jt");
	std::vector<std::shared_ptr<TemplateTask>> tasks = {mft, jt};
	RobotController rc(robot, tasks);
	BatchedSimulation sim(rc, 0.001, substeps);
	const Batch k(rows.begin(), rows.begin() + B), d(rows.begin() + B, rows.begin() + 2 * B), mu(rows.begin() + 2 * B, rows.end());
	expect_invalid("a body before the collision geometry", [&] { sim.setBodyContact(k, d, mu, categories, v_eps); });
	check(sim.robotsTouching() == 0 && sim.getBodyContactState().any == 0, "no contact before one is set");
	sim.setCollisionGeometry(links, centres, radii);
	sim.setCollisionEnvironment(P, O, env);
	sim.setBodyContact(k, d, mu, categories, v_eps);
	int cats = -1;
	check(sim.getBodyContact(&cats) == rows && cats == categories, "the rows and the categories in force");
	Batch out;
	int most = 0;
	for (int period = 0; period < periods; period++) {
		sim.setJointTorques(tau);
		sim.integrate();
		const Batch qn = sim.getJointPositions(), dqn = sim.getJointVelocities();
		const BodyContactState st = sim.getBodyContactState();
		out.insert(out.end(), qn.begin(), qn.end());
		out.insert(out.end(), dqn.begin(), dqn.end());
		out.insert(out.end(), st.status.begin(), st.status.end());
		for (int c : {st.plane, st.obstacle, st.self, st.any}) out.push_back((double)c);
		check(st.status.size() == (size_t)(9 + n) * sB && st.any == sim.robotsTouching() && st.any >= st.plane && st.any >= st.obstacle, "the state of a period");
		most = st.any > most ? st.any : most;
	}
	check(most >= B / 4, "a quarter of the robots touch");
	// the members' own exceptions leave the contact as it was
	expect_invalid("stiffness of another length", [&] { sim.setBodyContact(Batch(B - 1, 1.0)); });
	Batch bad = k;
	bad[B / 2] = -1.0;
	expect_invalid("a negative stiffness", [&] { sim.setBodyContact(bad, d, mu); });
	bad[B / 2] = NAN;
	expect_invalid("a NaN friction", [&] { sim.setBodyContact(k, d, bad); });
	expect_invalid("no category", [&] { sim.setBodyContact(k, d, mu, 0); });
	check(sim.getBodyContact(&cats) == rows && cats == categories, "a refused call changes nothing");
	sim.clearBodyContact();
	check(sim.getBodyContact(&cats) == Batch(3 * sB, 0.0) && cats == 0 && sim.robotsTouching() == 0, "clearBodyContact");
	sim.setBodyContact(k);
	sim.clearCollision();
	sim.getBodyContact(&cats);
	check(cats == 0, "clearCollision takes the body with it");
	// The sharded controller, two shards on one device: an explicit configuration (pairs whose links are at least 3 apart, so
	// that the self category can push too), every category, two periods stepped shard by shard; the gathered status and the summed
	// counts follow the single context's results in <out>.
	{
		sai2b_collision_config cfg = detail::collisionGeometry(n, links, centres, radii, SAI2B_COL_DISTANCE, 0.0, 0.0, 0.0, 0);
		cfg.n_planes = P, cfg.n_obstacles = O;
		for (int i = 0; i < SAI2B_MAX_COLLISION_SPHERES; i++) {
			cfg.pair_mask[i] = 0;
			for (int j = i + 1; j < S && i < S; j++)
				if (std::abs(links[i] - links[j]) >= 3) cfg.pair_mask[i] |= 1u << j;
		}
		ShardedRobotController sh(robot->model(), {mft->config(), jt->config()}, B, {0, 0});
		sh.setState(q, dq);
		expect_invalid("a sharded body before the collision configuration", [&] { sh.setBodyContact(rows); });
		sh.setCollision(cfg, env);
		expect_invalid("sharded rows of another shape", [&] { sh.setBodyContact(Batch(3 * sB - 1, 1.0)); });
		sh.setBodyContact(rows, detail::BODY_CONTACT_ALL, v_eps);
		for (int period = 0; period < 2; period++) {
			for (int s2 = 0; s2 < sh.shards(); s2++) {
				const std::pair<int, int> lohi = sh.shardBounds(s2);
				const size_t Bs = (size_t)(lohi.second - lohi.first);
				Batch part((size_t)n * Bs);
				for (int i = 0; i < n; i++)
					for (size_t b = 0; b < Bs; b++) part[i * Bs + b] = tau[i * sB + lohi.first + b];
				detail::check(sh.ctx(s2), sai2b_sim_step(sh.ctx(s2), part.data(), 0, 0.001, substeps, 0));
			}
			const BodyContactState st = sh.getBodyContactState();
			out.insert(out.end(), st.status.begin(), st.status.end());
			for (int c : {st.plane, st.obstacle, st.self, st.any}) out.push_back((double)c);
			check(st.status.size() == (size_t)(9 + n) * sB && st.any >= B / 4, "the sharded state of a period");
		}
		sh.clearBodyContact();
		check(sh.getBodyContactState().any == 0, "sharded clearBodyContact");
	}
	FILE* f = std::fopen(out_path, "wb");
	if (!f) return 2;
	const size_t put = std::fwrite(out.data(), sizeof(double), out.size(), f);
	std::fclose(f);
	check(put == out.size(), "results written");
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

int main(int argc, char** argv) {
	if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
	if (argc == 5 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3], argv[4]);
	std::fprintf(stderr, "usage: body_contact_facade_test validate | run <urdf> <in> <out>\n");
	return 2;
}

// The collision members of the C++ facade (include/Sai2PrimitivesBatched.h: setCollisionGeometry, setCollisionEnvironment,
// clearCollision, queryCollision, collisionCounts, endEpisodes on BatchedSimulation; setCollision, queryCollision, collisionCounts,
// endEpisodes on ShardedRobotController).
// `validate <urdf>` needs no device: the members by signature, the struct's size, link-name resolution (a body behind a fixed
// joint, the world), and the std::invalid_argument conditions that are judged ahead of the device. `run <urdf>`: on 130 Pandas a
// sphere on the end-effector body over a floor: the distance is the body's height minus the radius, the flags follow the margin,
// the counts add up; an obstacle placed on the sphere's centre gives the zero normal; endEpisodes closes what it should; the
// exceptions of the members themselves, which leave the configuration as it was; clearCollision.
#include <algorithm>
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

static int validate(const char* urdf) {
	using M = detail::CollisionMembers;
	static_assert(std::is_base_of<M, BatchedSimulation>::value, "BatchedSimulation has the members");
	static_assert(std::is_same<decltype(&M::setCollisionEnvironment), void (M::*)(int, int, const Batch&)>::value, "setCollisionEnvironment");
	static_assert(std::is_same<decltype(&M::clearCollision), void (M::*)()>::value, "clearCollision");
	static_assert(std::is_same<decltype(&M::queryCollision), CollisionResult (M::*)(bool)>::value, "queryCollision");
	static_assert(std::is_same<decltype(&M::collisionCounts), CollisionCounts (M::*)() const>::value, "collisionCounts");
	static_assert(std::is_same<decltype(&M::endEpisodes), int (M::*)(std::vector<unsigned char>&, const std::vector<unsigned char>&, int)>::value, "endEpisodes");
	using S = ShardedRobotController;
	static_assert(std::is_same<decltype(&S::setCollision), void (S::*)(const sai2b_collision_config&, const Batch&)>::value, "sharded setCollision");
	static_assert(std::is_same<decltype(&S::queryCollision), CollisionResult (S::*)()>::value, "sharded queryCollision");
	static_assert(std::is_same<decltype(&S::collisionCounts), CollisionCounts (S::*)()>::value, "sharded collisionCounts");
	static_assert(std::is_same<decltype(&S::endEpisodes), int (S::*)(std::vector<unsigned char>&, const std::vector<unsigned char>&, int)>::value, "sharded endEpisodes");
	static_assert(std::is_same<decltype(&S::clearCollision), void (S::*)()>::value, "sharded clearCollision");
	void (M::*by_index)(const std::vector<int>&, const std::vector<double>&, const std::vector<double>&, int, double, double, double, int) = &M::setCollisionGeometry;
	void (M::*by_name)(const BatchedRobotModel&, const std::vector<std::string>&, const std::vector<double>&, const std::vector<double>&, int, double, double,
					   double, int) = &M::setCollisionGeometry;
	check(by_index != nullptr && by_name != nullptr, "members compile");
	check(sai2b_sizeof_collision_config() == (int)sizeof(sai2b_collision_config), "size of the configuration");
	// link names: the end-effector body hangs on link7 behind a fixed joint 0.15 m up its z; an empty name is the world
	BatchedRobotModel robot(urdf, 4);
	std::vector<int> links;
	std::vector<double> in_model;
	detail::resolveCollisionSpheres(robot, {"link7", "end-effector", "", "link1"}, {0.01, 0.02, 0.03, 0, 0, 0.05, 0.4, 0.5, 0.6, 0, 0, 0}, &links, &in_model);
	check(links == std::vector<int>({6, 6, -1, 0}), "link names resolve to moving links and the world");
	check(in_model[0] == 0.01 && in_model[2] == 0.03 && std::fabs(in_model[5] - 0.2) < 1e-15 && in_model[3] == 0 && in_model[6] == 0.4 && in_model[8] == 0.6,
		  "centres are carried into the moving link's frame");
	expect_invalid("an unknown link name", [&] { detail::resolveCollisionSpheres(robot, {"link9"}, {0, 0, 0}, &links, &in_model); });
	expect_invalid("centres that do not fit the names", [&] { detail::resolveCollisionSpheres(robot, {"link1"}, {0, 0}, &links, &in_model); });
	BatchedRobotModel no_urdf(4);
	expect_invalid("link names without a URDF", [&] { detail::resolveCollisionSpheres(no_urdf, {"link1"}, {0, 0, 0}, &links, &in_model); });
	// the geometry, judged without a device
	const sai2b_collision_config cfg = detail::collisionGeometry(7, {-1, 0, 2, 6}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.1}, {0.1, 0.1, 0.1, 0.05},
																 SAI2B_COL_DISTANCE | SAI2B_COL_GRADIENT, 0.1, 0.2, 0.3, 1);
	check(cfg.n_spheres == 4 && cfg.env_mask == 0xEu && cfg.pair_mask[0] == 0xCu && cfg.pair_mask[1] == 0xCu && cfg.pair_mask[2] == 0x8u && cfg.view == 1 &&
			  cfg.margin_self == 0.3,
		  "the default masks");
	expect_invalid("no sphere", [&] { detail::collisionGeometry(7, {}, {}, {}, 1, 0, 0, 0, 0); });
	expect_invalid("17 spheres", [&] { detail::collisionGeometry(7, std::vector<int>(17, 0), std::vector<double>(51, 0), std::vector<double>(17, 0), 1, 0, 0, 0, 0); });
	expect_invalid("centres of another length", [&] { detail::collisionGeometry(7, {0, 1}, {0, 0, 0}, {0.1, 0.1}, 1, 0, 0, 0, 0); });
	expect_invalid("a link beyond the robot", [&] { detail::collisionGeometry(7, {7}, {0, 0, 0}, {0.1}, 1, 0, 0, 0, 0); });
	expect_invalid("a negative radius", [&] { detail::collisionGeometry(7, {0}, {0, 0, 0}, {-0.1}, 1, 0, 0, 0, 0); });
	expect_invalid("unknown blocks", [&] { detail::collisionGeometry(7, {0}, {0, 0, 0}, {0.1}, 64, 0, 0, 0, 0); });
	expect_invalid("a margin that is not finite", [&] { detail::collisionGeometry(7, {0}, {0, 0, 0}, {0.1}, 1, NAN, 0, 0, 0); });
	expect_invalid("view 2", [&] { detail::collisionGeometry(7, {0}, {0, 0, 0}, {0.1}, 1, 0, 0, 0, 2); });
	expect_invalid("three planes", [&] { detail::checkCollisionEnvironment(3, 0, 4, {}); });
	expect_invalid("rows of another shape", [&] { detail::checkCollisionEnvironment(1, 1, 4, Batch(39)); });
	detail::checkCollisionEnvironment(1, 1, 4, Batch(40));
	detail::checkCollisionEnvironment(2, 4, 4, {});
	expect_invalid("bit 32", [&] { detail::checkEndEpisodes(4, std::vector<unsigned char>(4), std::vector<unsigned char>(4), 32); });
	expect_invalid("extra of another length", [&] { detail::checkEndEpisodes(4, std::vector<unsigned char>(4), std::vector<unsigned char>(3), 64); });
	detail::checkEndEpisodes(4, std::vector<unsigned char>(4), std::vector<unsigned char>(4), 128);
	check(sai2b_set_collision(nullptr, &cfg, nullptr, 0) == SAI2B_INVALID_ARGUMENT && sai2b_collision_query(nullptr, nullptr, nullptr, 0) == SAI2B_INVALID_ARGUMENT,
		  "the C calls reject a NULL context");
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

static int run(const char* urdf) {
	const int B = 130, n = 7;
	const size_t sB = (size_t)B;
	auto robot = std::make_shared<BatchedRobotModel>(urdf, B, 0);
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5};
	Batch q(n * sB), dq(n * sB, 0.0);
	for (int b = 0; b < B; b++)
		for (int i = 0; i < n; i++) q[i * sB + b] = q0[i] + 0.3 * std::sin(0.37 * b + i);
	robot->setQ(q);
	robot->setDq(dq);
	robot->updateModel();
	const double fp[3] = {0.0, 0.0, 0.15};
	auto mft = std::make_shared<MotionForceTask>(robot, "end-effector", fp);
	auto jt = std::make_shared<JointTask>(robot, "jt");
	std::vector<std::shared_ptr<TemplateTask>> tasks = {mft, jt};
	RobotController rc(robot, tasks);
	BatchedSimulation sim(rc, 0.001, 1);
	// where the sphere is: the control point of the task sits at the same point of the same body
	const Batch x = mft->getCurrentPosition();
	expect_invalid("the environment before the geometry", [&] { sim.setCollisionEnvironment(1, 0); });
	expect_invalid("a query before the geometry", [&] { sim.queryCollision(); });
	const double radius = 0.04;
	const std::vector<std::string> names = {"end-effector", "link4", ""};
	const std::vector<double> in_links = {0, 0, 0.15, 0, 0, 0, 0, 0, -2.0}, radii = {radius, 0.05, 0.1};
	const int blocks = SAI2B_COL_DISTANCE | SAI2B_COL_INDEX | SAI2B_COL_NORMAL | SAI2B_COL_CENTRES;
	sim.setCollisionGeometry(*robot, names, in_links, radii, blocks);
	// a floor at z = 0 for every robot but every tenth, which has none; one obstacle on the first sphere's centre
	Batch rows(10 * sB, 0.0);
	for (int b = 0; b < B; b++) {
		rows[5 * sB + b] = 1.0;
		if (b % 10 == 9) rows[2 * sB + b] = NAN;
		for (int a = 0; a < 3; a++) rows[(6 + a) * sB + b] = x[a * sB + b];
		rows[9 * sB + b] = 0.01;
	}
	sim.setCollisionEnvironment(1, 1, rows);
	check(sim.collisionRows() == 3 + 3 + 9 + 9, "rows of the selected blocks");
	// the plane margin: between the two middle clearances of the batch, so that about half the robots are flagged
	double margin;
	{
		const CollisionResult first = sim.queryCollision();
		std::vector<double> d;
		for (int b = 0; b < B; b++)
			if (b % 10 != 9) d.push_back(first.rows[b]);
		std::sort(d.begin(), d.end());
		margin = 0.5 * (d[d.size() / 2 - 1] + d[d.size() / 2]);
		check(d[d.size() / 2] - d[d.size() / 2 - 1] > 1e-9, "the margin is clear of every robot's distance");
	}
	sim.setCollisionGeometry(*robot, names, in_links, radii, blocks, margin, 0.0, 0.0);
	const CollisionResult r = sim.queryCollision();
	bool dist = true, flags = true, normal = true, centres = true;
	int flagged = 0, obstacle = 0;
	for (int b = 0; b < B; b++) {
		const bool floor = b % 10 != 9;
		const double lower = std::fmin(x[2 * sB + b] - radius, r.rows[(15 + 3 + 2) * sB + b] - 0.05);  // the end-effector's or link4's sphere
		const double d = r.rows[0 * sB + b];
		dist = dist && (floor ? std::fabs(d - lower) < 1e-12 : std::isinf(d)) && (floor ? r.rows[3 * sB + b] >= 0 : r.rows[3 * sB + b] == -1);
		normal = normal && r.rows[8 * sB + b] == (floor ? 1.0 : 0.0);
		for (int a = 0; a < 3; a++) centres = centres && std::fabs(r.rows[(15 + a) * sB + b] - x[a * sB + b]) < 1e-12;
		// the obstacle sits on the first sphere's centre: distance -r - r_o, and the norm that would be normalised is 0 to rounding
		const bool hit = floor && d < margin;
		flags = flags && ((r.flags[b] & 1) != 0) == hit && (r.flags[b] & 2) != 0;
		flagged += hit, obstacle += (r.flags[b] & 2) != 0;
	}
	check(dist, "plane distance is the lower sphere's height minus its radius; none without a floor");
	check(normal, "the witness normal is the floor's");
	check(centres, "the world centre of the sphere is the task's control point");
	check(flags && flagged > 0 && flagged < B, "flags follow the margins");
	const CollisionCounts c = sim.collisionCounts();
	check(c.plane == flagged && c.obstacle == obstacle && c.obstacle == B && c.any == B && c.nonfinite == 0, "counts");
	check(r.rows[2 * sB] > 0 && r.rows[5 * sB] == 16 * 0 + 1, "self: the nearest default pair is the end-effector's sphere and link4's");
	// the geometry again keeps the environment
	sim.setCollisionGeometry(*robot, {"end-effector"}, {0, 0, 0.15}, {radius}, SAI2B_COL_DISTANCE, margin);
	const CollisionResult r2 = sim.queryCollision();
	bool kept = sim.collisionRows() == 3;
	for (int b = 0; b < B; b++) kept = kept && (b % 10 == 9 ? std::isinf(r2.rows[b]) : std::fabs(r2.rows[b] - (x[2 * sB + b] - radius)) < 1e-12);
	check(kept, "a new geometry keeps the planes and obstacles");
	check(sim.queryCollision(false).rows.empty(), "flags alone");
	// exceptions of the members themselves leave the configuration as it was
	Batch bad = rows;
	bad[3 * sB + 5] = 0.5;
	expect_invalid("a normal that is not a unit vector", [&] { sim.setCollisionEnvironment(1, 1, bad); });
	expect_invalid("rows of another shape", [&] { sim.setCollisionEnvironment(1, 1, Batch(9 * sB)); });
	expect_invalid("a link name that does not exist", [&] { sim.setCollisionGeometry(*robot, {"link9"}, {0, 0, 0}, {0.1}); });
	const CollisionResult r3 = sim.queryCollision();
	check(r3.rows.size() == r2.rows.size() && std::memcmp(r3.rows.data(), r2.rows.data(), r2.rows.size() * sizeof(double)) == 0 && r3.flags == r2.flags,
		  "a rejected call changes nothing");
	// endEpisodes
	std::vector<unsigned char> done(B, 0), extra = r3.flags;
	for (int b = 0; b < B; b += 3) done[b] = SAI2B_DONE_SPEED;
	expect_invalid("endEpisodes bit 1", [&] { sim.endEpisodes(done, extra, 1); });
	expect_invalid("endEpisodes with a short mask", [&] {
		std::vector<unsigned char> small(B - 1);
		sim.endEpisodes(done, small);
	});
	int want = 0;
	bool bytes = true;
	std::vector<unsigned char> before = done;
	const int closed = sim.endEpisodes(done, extra);
	for (int b = 0; b < B; b++) {
		want += extra[b] && !before[b];
		bytes = bytes && done[b] == (extra[b] ? (before[b] | SAI2B_DONE_COLLISION) : before[b]);
	}
	check(closed == want && bytes && want > 0, "endEpisodes marks the selected robots and counts those it closed");
	sim.clearCollision();
	check(sim.collisionRows() == -1, "clearCollision");
	expect_invalid("a query after clearCollision", [&] { sim.queryCollision(); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

int main(int argc, char** argv) {
	if (argc == 3 && !std::strcmp(argv[1], "validate")) return validate(argv[2]);
	if (argc == 3 && !std::strcmp(argv[1], "run")) return run(argv[2]);
	std::fprintf(stderr, "usage: collision_facade_test validate|run <panda urdf>\n");
	return 2;
}

// Snapshot banks through the C++ facade (include/Sai2PrimitivesBatched.h: SnapshotBank, RobotController::createSnapshotBank,
// BatchedSimulation::createSnapshotBank). `validate` needs no device: the members by signature, the size checks made ahead of
// the device, the C entry points' treatment of NULL. `run`: the round trip and the clone on 130 robots against a twin controller
// that is never interrupted, bit for bit, and std::invalid_argument for a blob of another hierarchy.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "Sai2PrimitivesBatched.h"

using namespace Sai2Primitives;
using Mask = std::vector<unsigned char>;
using Slots = std::vector<int>;

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

static int validate() {
	static_assert(std::is_same<decltype(&RobotController::createSnapshotBank), std::unique_ptr<SnapshotBank> (RobotController::*)(int, int)>::value,
				  "RobotController::createSnapshotBank(capacity, what)");
	static_assert(std::is_same<decltype(&BatchedSimulation::createSnapshotBank), std::unique_ptr<SnapshotBank> (BatchedSimulation::*)(int, int)>::value,
				  "BatchedSimulation::createSnapshotBank(capacity, what)");
	static_assert(std::is_same<decltype(&SnapshotBank::save), void (SnapshotBank::*)(const Slots&, const Mask&)>::value, "SnapshotBank::save");
	static_assert(std::is_same<decltype(&SnapshotBank::load), void (SnapshotBank::*)(const Slots&, const Mask&)>::value, "SnapshotBank::load");
	static_assert(std::is_same<decltype(&SnapshotBank::counts), SnapshotCounts (SnapshotBank::*)() const>::value, "SnapshotBank::counts");
	static_assert(std::is_same<decltype(&SnapshotBank::exportBlob), std::vector<unsigned char> (SnapshotBank::*)()>::value, "SnapshotBank::exportBlob");
	static_assert(std::is_same<decltype(&SnapshotBank::importBlob), void (SnapshotBank::*)(const std::vector<unsigned char>&)>::value,
				  "SnapshotBank::importBlob");
	static_assert(!std::is_copy_constructible<SnapshotBank>::value, "a bank owns device memory");
	check(true, "members compile");
	// the C entry points reject NULL before anything touches a device
	sai2b_snapshot_bank* bank = nullptr;
	int counts[3];
	unsigned char blob[SAI2B_SNAPSHOT_HEADER_BYTES] = {};
	check(sai2b_snapshot_bank_create(nullptr, 4, SAI2B_SNAP_EPISODE, &bank) == SAI2B_INVALID_ARGUMENT && !bank, "sai2b_snapshot_bank_create(NULL ctx)");
	check(sai2b_snapshot_save(nullptr, nullptr, nullptr, nullptr, 0) == SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_save(NULL ctx)");
	check(sai2b_snapshot_load(nullptr, nullptr, nullptr, nullptr, 0) == SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_load(NULL ctx)");
	check(sai2b_get_snapshot_counts(nullptr, counts) == SAI2B_INVALID_ARGUMENT, "sai2b_get_snapshot_counts(NULL ctx)");
	check(sai2b_snapshot_words(nullptr, SAI2B_SNAP_EPISODE) == -1, "sai2b_snapshot_words(NULL ctx)");
	check(sai2b_snapshot_export_size(nullptr) == 0, "sai2b_snapshot_export_size(NULL bank)");
	check(sai2b_snapshot_export(nullptr, blob, sizeof(blob)) == SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_export(NULL bank)");
	check(sai2b_snapshot_import(nullptr, blob, sizeof(blob)) == SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_import(NULL bank)");
	sai2b_snapshot_bank_destroy(nullptr);
	check(true, "sai2b_snapshot_bank_destroy(NULL bank)");
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

// a controller of one full JointTask (generator on, integral gain on) with its plant
struct Rig {
	std::shared_ptr<BatchedRobotModel> robot;
	std::shared_ptr<JointTask> jt;
	std::unique_ptr<RobotController> rc;
	std::unique_ptr<BatchedSimulation> sim;
	int B;
	Rig(const sai2b_robot_model& model, int batch) : B(batch) {
		robot = std::make_shared<BatchedRobotModel>(batch, model, 0);
		jt = std::make_shared<JointTask>(robot, "jt");
		std::vector<std::shared_ptr<TemplateTask>> tasks = {jt};
		rc = std::make_unique<RobotController>(robot, tasks);
		sim = std::make_unique<BatchedSimulation>(*rc);
		sai2b_task_config cfg;
		detail::check(nullptr, sai2b_default_joint_task(&cfg, "jt", 7, nullptr));
		for (int i = 0; i < 7; i++) cfg.ki[i] = 3.0;
		detail::check(rc->ctx(), sai2b_update_task_config(rc->ctx(), 0, &cfg));
	}
	void start(const Batch& q, const Batch& dq, const Batch& goal) {
		detail::check(rc->ctx(), sai2b_set_state(rc->ctx(), q.data(), dq.data(), 0));
		rc->reinitializeTasks();
		goals(goal);
	}
	void goals(const Batch& goal) { detail::check(rc->ctx(), sai2b_set_jt_goals(rc->ctx(), 0, goal.data(), nullptr, nullptr, 0)); }
	// torques, then the state after the step
	Batch period() {
		Batch out = rc->tick();
		sim->integrate();
		const Batch q = sim->getJointPositions(), dq = sim->getJointVelocities();
		out.insert(out.end(), q.begin(), q.end());
		out.insert(out.end(), dq.begin(), dq.end());
		return out;
	}
};

static bool same_bits(const Batch& a, const Batch& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

static int run() {
	const int B = 130, n = 7;
	sai2b_robot_model model;
	detail::check(nullptr, sai2b_panda_model(&model));
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5};
	Batch q(n * (size_t)B), dq(n * (size_t)B), goal(n * (size_t)B), goal2(n * (size_t)B);
	for (int b = 0; b < B; b++)
		for (int i = 0; i < n; i++) {
			const size_t k = i * (size_t)B + b;
			q[k] = q0[i] + 0.3 * std::sin(0.37 * b + i), dq[k] = 0.2 * std::cos(0.11 * b + 2 * i);
			goal[k] = q[k] + 0.1 * std::sin(0.7 * b + 3 * i), goal2[k] = q[k] - 0.15 * std::cos(0.3 * b + i);
		}
	Rig a(model, B), twin(model, B);
	bool ok = true;
	for (Rig* r : {&a, &twin}) r->start(q, dq, goal);
	for (int k = 0; k < 20; k++) ok = same_bits(a.period(), twin.period()) && ok;
	check(ok, "history bit-equal");

	// round trip, through the bank of the simulation (both groups)
	auto bank = a.sim->createSnapshotBank(B);
	check(throws_invalid([&] { bank->save(Slots(B - 1, 0)); }), "save: wrong slots length");
	check(throws_invalid([&] { bank->load({}, Mask(B + 1, 1)); }), "load: wrong mask length");
	bank->save();
	SnapshotCounts c = bank->counts();
	check(c.moved == B && c.out_of_range == 0 && c.never_saved == 0, "save counts");
	a.goals(goal2);
	Batch last;
	for (int k = 0; k < 5; k++) last = a.period();
	bank->load();
	c = bank->counts();
	check(c.moved == B && c.out_of_range == 0 && c.never_saved == 0, "load counts");
	ok = true;
	Batch first;
	for (int k = 0; k < 10; k++) {
		const Batch x = a.period(), y = twin.period();
		if (k == 0) first = y;
		ok = same_bits(x, y) && ok;
	}
	check(ok, "round trip bit-equal to the twin");
	check(!same_bits(last, first), "the detour was one");

	// clone: robot 70 into slot 0 of a bank of one slot, slot 0 into every robot
	auto one = a.rc->createSnapshotBank(1);
	Mask only(B, 0);
	only[70] = 1;
	one->save(Slots(B, 0), only);
	c = one->counts();
	check(c.moved == 1 && c.out_of_range == 0, "clone: one robot saved");
	Slots bad(B, 0);
	bad[3] = 1, bad[4] = -1;
	one->load(bad);
	c = one->counts();
	check(c.moved == B - 2 && c.out_of_range == 2 && c.never_saved == 0, "clone: slots out of range are counted");
	one->load(Slots(B, 0));
	ok = true;
	for (int k = 0; k < 5; k++) {
		const Batch x = a.period(), y = twin.period();
		for (size_t row = 0; row < x.size() / B; row++)
			for (int b = 0; b < B; b++) ok = ok && std::memcmp(&x[row * B + b], &y[row * B + 70], sizeof(double)) == 0;
	}
	check(ok, "clone: every column is robot 70 of the twin");

	// checkpoint through the facade, and a blob of another hierarchy
	const std::vector<unsigned char> blob = bank->exportBlob();
	check(blob.size() == sai2b_snapshot_export_size(bank->handle()) && blob.size() > SAI2B_SNAPSHOT_HEADER_BYTES, "export size");
	{
		Rig fresh(model, B);
		auto again = fresh.sim->createSnapshotBank(B);
		again->importBlob(blob);
		again->load();
		Rig ref(model, B);
		ref.start(q, dq, goal);
		for (int k = 0; k < 20; k++) ref.period();
		ok = true;
		for (int k = 0; k < 5; k++) ok = same_bits(fresh.period(), ref.period()) && ok;
		check(ok, "import into a fresh controller continues bit-equal");
		check(throws_invalid([&] { again->importBlob(std::vector<unsigned char>(blob.begin(), blob.end() - 1)); }), "truncated blob");
	}
	{
		std::vector<sai2b_task_config> cfgs(2);
		const double fp[3] = {0, 0, 0.1};
		detail::check(nullptr, sai2b_default_motion_force_task(&cfgs[0], "mft", 6, fp, nullptr, -1, nullptr, -1, nullptr));
		detail::check(nullptr, sai2b_default_joint_task(&cfgs[1], "jt", 7, nullptr));
		sai2b_ctx* other = sai2b_create(&model, cfgs.data(), 2, B, 0);
		if (!other) throw std::runtime_error(sai2b_last_error(nullptr));
		{
			SnapshotBank foreign(other, B, SAI2B_SNAP_EPISODE | SAI2B_SNAP_ENVIRONMENT);
			std::string msg;
			try {
				foreign.importBlob(blob);
			} catch (const std::invalid_argument& e) {
				msg = e.what();
			}
			check(msg.find("block") != std::string::npos, "foreign blob: std::invalid_argument naming the block");
		}
		sai2b_destroy(other);
	}
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
	std::printf("usage: snapshot_facade_test validate|run\n");
	return 2;
}

// The contact members of BatchedSimulation (include/Sai2PrimitivesBatched.h) compile against the C ABI, and the checks that
// setContactPlanes makes ahead of the device (BatchedSimulation::checkContactArguments: every condition sai2b_set_contact puts
// on host arguments) throw std::invalid_argument; the sensor-task conditions, which the facade cannot violate (it takes a
// MotionForceTask object), through sai2b_validate_contact.
// Usage: contact_facade_test validate
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
// what sai2b_set_contact does with a configuration before it touches the device
static void validate(sai2b_contact_config cfg, const sai2b_task_config* tasks, int n_tasks) {
	char msg[256];
	if (sai2b_validate_contact(&cfg, tasks, n_tasks, SAI2B_DOF, msg, sizeof(msg)) == SAI2B_INVALID_ARGUMENT) throw std::invalid_argument(msg);
}

int main(int argc, char** argv) {
	if (argc < 2 || std::strcmp(argv[1], "validate") != 0) {
		std::fprintf(stderr, "usage: %s validate\n", argv[0]);
		return 2;
	}
	// the members exist with these signatures (never called: there is no device here)
	void (BatchedSimulation::*by_index)(int, const std::vector<double>&, const Batch&, const Batch&, const Batch&, const Batch&, const Batch&,
										double) = &BatchedSimulation::setContactPlanes;
	void (BatchedSimulation::*by_name)(const BatchedRobotModel&, const std::string&, const std::vector<double>&, const Batch&, const Batch&,
									   const Batch&, const Batch&, const Batch&, double) = &BatchedSimulation::setContactPlanes;
	void (BatchedSimulation::*attach)(const MotionForceTask&) = &BatchedSimulation::attachForceSensor;
	void (BatchedSimulation::*clear)() = &BatchedSimulation::clearContact;
	BatchedSimulation::ContactState (BatchedSimulation::*state)() const = &BatchedSimulation::getContactState;
	int (BatchedSimulation::*count)() const = &BatchedSimulation::robotsInContact;
	if (!by_index || !by_name || !attach || !clear || !state || !count) return 3;

	// the checks setContactPlanes makes before it touches the device, on a two-robot batch of a 7-joint robot
	const size_t B = 2;
	const std::vector<double> tip = {0.0, 0.0, 0.1};
	const Batch p0(3 * B, 0.0), k(B, 1e3), none;
	Batch n(3 * B, 0.0);
	n[2 * B] = n[2 * B + 1] = 1.0;
	auto check = [&](int link, const std::vector<double>& pts, const Batch& pp, const Batch& pn, const Batch& ks, const Batch& d, const Batch& mu,
					 double eps) { BatchedSimulation::checkContactArguments(7, B, link, pts, pp, pn, ks, d, mu, eps); };
	check(6, tip, p0, n, k, none, none, 1e-3);	// accepted
	auto edited = [](Batch a, size_t i, double v) {
		a[i] = v;
		return a;
	};
	expect_invalid("link below 0", [&] { check(-1, tip, p0, n, k, none, none, 1e-3); });
	expect_invalid("link == dof", [&] { check(7, tip, p0, n, k, none, none, 1e-3); });
	expect_invalid("no points", [&] { check(6, {}, p0, n, k, none, none, 1e-3); });
	expect_invalid("five points", [&] { check(6, std::vector<double>(15, 0.0), p0, n, k, none, none, 1e-3); });
	expect_invalid("points not n x 3", [&] { check(6, {0.0, 0.0, 0.1, 0.2}, p0, n, k, none, none, 1e-3); });
	expect_invalid("non-finite point", [&] { check(6, {0.0, NAN, 0.1}, p0, n, k, none, none, 1e-3); });
	expect_invalid("v_eps 0", [&] { check(6, tip, p0, n, k, none, none, 0.0); });
	expect_invalid("rows of the wrong size", [&] { check(6, tip, Batch(3), n, k, none, none, 1e-3); });
	expect_invalid("non-finite plane point", [&] { check(6, tip, edited(p0, 1, INFINITY), n, k, none, none, 1e-3); });
	expect_invalid("normal not of unit length", [&] { check(6, tip, p0, edited(n, 2 * B, 1.001), k, none, none, 1e-3); });
	expect_invalid("negative stiffness", [&] { check(6, tip, p0, n, edited(k, 1, -1.0), none, none, 1e-3); });
	expect_invalid("negative damping", [&] { check(6, tip, p0, n, k, Batch(B, -0.1), none, 1e-3); });
	expect_invalid("negative friction", [&] { check(6, tip, p0, n, k, none, Batch(B, -0.1), 1e-3); });

	sai2b_task_config tasks[2];
	sai2b_default_motion_force_task(&tasks[0], "m", 6, nullptr, nullptr, -1, nullptr, -1, nullptr);
	sai2b_default_joint_task(&tasks[1], "j", 0, nullptr);
	sai2b_contact_config ok;
	const double pts[6] = {0.01, 0, 0.1, -0.01, 0, 0.1};
	if (sai2b_default_contact(&ok, 6, 2, pts) != SAI2B_OK) return 4;
	ok.sensor_task = 0;
	validate(ok, tasks, 2);	 // accepted
	auto with = [&](const std::function<void(sai2b_contact_config&)>& edit) {
		sai2b_contact_config c = ok;
		edit(c);
		return c;
	};
	// the sensor task is given to the facade as a MotionForceTask object, so only the C ABI can name a wrong one
	expect_invalid("sensor on a JointTask", [&] { validate(with([](sai2b_contact_config& c) { c.sensor_task = 1; }), tasks, 2); });
	expect_invalid("sensor past the tasks", [&] { validate(with([](sai2b_contact_config& c) { c.sensor_task = 2; }), tasks, 2); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

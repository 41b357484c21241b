// The external-wrench members of BatchedSimulation (include/Sai2PrimitivesBatched.h) compile against the C ABI, and the checks
// that setExternalWrench makes ahead of the device (BatchedSimulation::checkExternalWrenchArguments: every condition
// sai2b_set_external_wrench puts on host arguments) throw std::invalid_argument; the sensor-task conditions, which the facade
// cannot violate (it takes a MotionForceTask object), through sai2b_validate_external_wrench.
// Usage: external_wrench_facade_test validate
#include <array>
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
// what sai2b_set_external_wrench does with a configuration before it touches the device
static void validate(sai2b_external_wrench_config cfg, const sai2b_task_config* tasks, int n_tasks) {
	char msg[256];
	if (sai2b_validate_external_wrench(&cfg, tasks, n_tasks, SAI2B_DOF, msg, sizeof(msg)) == SAI2B_INVALID_ARGUMENT) throw std::invalid_argument(msg);
}

int main(int argc, char** argv) {
	if (argc < 2 || std::strcmp(argv[1], "validate") != 0) {
		std::fprintf(stderr, "usage: %s validate\n", argv[0]);
		return 2;
	}
	// the members exist with these signatures (never called: there is no device here)
	using Point = std::array<double, 3>;
	void (BatchedSimulation::*by_index)(int, const Batch&, const Batch&, const Batch&, const Point&, int, const MotionForceTask*) =
		&BatchedSimulation::setExternalWrench;
	void (BatchedSimulation::*by_name)(const BatchedRobotModel&, const std::string&, const Point&, const Batch&, const Batch&, const Batch&, int,
									   const MotionForceTask*) = &BatchedSimulation::setExternalWrench;
	void (BatchedSimulation::*clear)() = &BatchedSimulation::clearExternalWrench;
	BatchedSimulation::ExternalWrenchState (BatchedSimulation::*state)() const = &BatchedSimulation::getExternalWrenchState;
	int (BatchedSimulation::*count)() const = &BatchedSimulation::robotsPushed;
	if (!by_index || !by_name || !clear || !state || !count) return 3;
	if (sai2b_sizeof_external_wrench_config() != (int)sizeof(sai2b_external_wrench_config)) return 5;

	// the checks setExternalWrench makes before it touches the device, on a two-robot batch of a 7-joint robot
	const size_t B = 2;
	const Point tip = {0.0, 0.0, 0.1};
	const Batch F(3 * B, 5.0), M(3 * B, 0.5), S(B, 3.0), none;
	auto check = [&](int link, const Batch& f, const Batch& m, const Batch& s, const Point& c, int frame) {
		BatchedSimulation::checkExternalWrenchArguments(7, B, link, f, m, s, c, frame);
	};
	check(6, F, M, S, tip, SAI2B_WRENCH_LINK);	   // accepted
	check(0, F, none, none, tip, SAI2B_WRENCH_WORLD);  // accepted: no moment, pushed until changed
	auto edited = [](Batch a, size_t i, double v) {
		a[i] = v;
		return a;
	};
	expect_invalid("link below 0", [&] { check(-1, F, M, S, tip, SAI2B_WRENCH_WORLD); });
	expect_invalid("link == dof", [&] { check(7, F, M, S, tip, SAI2B_WRENCH_WORLD); });
	expect_invalid("unknown frame", [&] { check(6, F, M, S, tip, 2); });
	expect_invalid("non-finite point", [&] { check(6, F, M, S, Point{0.0, NAN, 0.1}, SAI2B_WRENCH_WORLD); });
	expect_invalid("no force", [&] { check(6, none, M, S, tip, SAI2B_WRENCH_WORLD); });
	expect_invalid("force of the wrong size", [&] { check(6, Batch(3), M, S, tip, SAI2B_WRENCH_WORLD); });
	expect_invalid("moment of the wrong size", [&] { check(6, F, Batch(B), S, tip, SAI2B_WRENCH_WORLD); });
	expect_invalid("steps of the wrong size", [&] { check(6, F, M, Batch(3 * B), tip, SAI2B_WRENCH_WORLD); });
	expect_invalid("non-finite force", [&] { check(6, edited(F, 1, INFINITY), M, S, tip, SAI2B_WRENCH_WORLD); });
	expect_invalid("non-finite moment", [&] { check(6, F, edited(M, 5, NAN), S, tip, SAI2B_WRENCH_WORLD); });
	expect_invalid("NaN steps", [&] { check(6, F, M, edited(S, 1, NAN), tip, SAI2B_WRENCH_WORLD); });
	check(6, F, M, edited(S, 1, INFINITY), tip, SAI2B_WRENCH_WORLD);  // accepted: an infinite count is a count

	// the by-name overload turns link-frame rows from the named link's frame into the moving link's: a quarter turn about z
	{
		const double Rz[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
		const Batch rows = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0};	// [3][2]: robot 0 (1, 3, 5), robot 1 (2, 4, 6)
		const Batch want = {-3.0, -4.0, 1.0, 2.0, 5.0, 6.0};
		if (BatchedSimulation::turnedRows(Rz, rows) != want || !BatchedSimulation::turnedRows(Rz, none).empty() ||
			BatchedSimulation::turnedRows(Rz, Batch(4, 1.0)).size() != 4) {
			std::printf("FAIL turnedRows\n");
			failures++;
		}
	}

	sai2b_task_config tasks[2];
	sai2b_default_motion_force_task(&tasks[0], "m", 6, nullptr, nullptr, -1, nullptr, -1, nullptr);
	sai2b_default_joint_task(&tasks[1], "j", 0, nullptr);
	sai2b_external_wrench_config ok;
	if (sai2b_default_external_wrench(&ok, 6) != SAI2B_OK) return 4;
	if (ok.link != 6 || ok.frame != SAI2B_WRENCH_WORLD || ok.sensor_task != -1 || ok.point[0] != 0 || ok.point[1] != 0 || ok.point[2] != 0) return 6;
	ok.sensor_task = 0;
	validate(ok, tasks, 2);	 // accepted
	auto with = [&](const std::function<void(sai2b_external_wrench_config&)>& edit) {
		sai2b_external_wrench_config c = ok;
		edit(c);
		return c;
	};
	// the sensor task is given to the facade as a MotionForceTask object, so only the C ABI can name a wrong one
	expect_invalid("sensor on a JointTask", [&] { validate(with([](sai2b_external_wrench_config& c) { c.sensor_task = 1; }), tasks, 2); });
	expect_invalid("sensor past the tasks", [&] { validate(with([](sai2b_external_wrench_config& c) { c.sensor_task = 2; }), tasks, 2); });
	expect_invalid("sensor below -1", [&] { validate(with([](sai2b_external_wrench_config& c) { c.sensor_task = -2; }), tasks, 2); });
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

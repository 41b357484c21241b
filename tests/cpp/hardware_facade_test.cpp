// The hardware members of BatchedSimulation (include/Sai2PrimitivesBatched.h: setHardware, clearHardware, getHardwareState).
// `validate` needs no device: the members by signature, the struct's size, and the sensor-task conditions, which the facade
// cannot violate (it takes a MotionForceTask object), through sai2b_validate_hardware. `run`: on 130 Pandas, setHardware with a
// delay, a gain and a sensor task through 6 periods of integrate() against the known delayed command; the sensor's bias on
// the reading of an external wrench against a twin without hardware; clearHardware back to the ideal path; and
// std::invalid_argument from setHardware itself.
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
static void validate_config(sai2b_hardware_config cfg, const sai2b_task_config* tasks, int n_tasks) {
	char msg[256];
	if (sai2b_validate_hardware(&cfg, tasks, n_tasks, SAI2B_DOF, msg, sizeof(msg)) == SAI2B_INVALID_ARGUMENT) throw std::invalid_argument(msg);
}

static int validate() {
	static_assert(std::is_same<decltype(&BatchedSimulation::setHardware),
							   void (BatchedSimulation::*)(const Batch&, const Batch&, int, const MotionForceTask*, unsigned long long, unsigned)>::value,
				  "BatchedSimulation::setHardware");
	static_assert(std::is_same<decltype(&BatchedSimulation::clearHardware), void (BatchedSimulation::*)()>::value, "BatchedSimulation::clearHardware");
	static_assert(std::is_same<decltype(&BatchedSimulation::getHardwareState), BatchedSimulation::HardwareState (BatchedSimulation::*)() const>::value,
				  "BatchedSimulation::getHardwareState");
	check(true, "members compile");
	check(sai2b_sizeof_hardware_config() == (int)sizeof(sai2b_hardware_config), "size of the configuration");
	sai2b_task_config tasks[2];
	sai2b_default_motion_force_task(&tasks[0], "m", 6, nullptr, nullptr, -1, nullptr, -1, nullptr);
	sai2b_default_joint_task(&tasks[1], "j", 0, nullptr);
	sai2b_hardware_config ok;
	check(sai2b_default_hardware(&ok) == SAI2B_OK && ok.max_delay == 0 && ok.sensor_task == -1 && ok.first_robot == 0 && ok.seed == 0, "defaults");
	ok.sensor_task = 0;
	validate_config(ok, tasks, 2);	// accepted
	auto with = [&](int task) {
		sai2b_hardware_config c = ok;
		c.sensor_task = task;
		return c;
	};
	expect_invalid("sensor on a JointTask", [&] { validate_config(with(1), tasks, 2); });
	expect_invalid("sensor past the tasks", [&] { validate_config(with(2), tasks, 2); });
	expect_invalid("sensor below -1", [&] { validate_config(with(-2), tasks, 2); });
	check(sai2b_set_hardware(nullptr, &ok, nullptr, nullptr, 0) == SAI2B_INVALID_ARGUMENT, "sai2b_set_hardware(NULL ctx)");
	check(sai2b_clear_hardware(nullptr) == SAI2B_INVALID_ARGUMENT, "sai2b_clear_hardware(NULL ctx)");
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

// [MotionForceTask on the last link, JointTask] with its plant, an external wrench read by the MotionForceTask's sensor
struct Rig {
	std::shared_ptr<BatchedRobotModel> robot;
	std::shared_ptr<MotionForceTask> mft;
	std::shared_ptr<JointTask> jt;
	std::unique_ptr<RobotController> rc;
	std::unique_ptr<BatchedSimulation> sim;
	Rig(const sai2b_robot_model& model, int B, const Batch& q, const Batch& dq, const Batch& force) {
		robot = std::make_shared<BatchedRobotModel>(B, model, 0);
		const double fp[3] = {0.0, 0.0, 0.1};
		mft = std::make_shared<MotionForceTask>(robot, 6, fp);
		jt = std::make_shared<JointTask>(robot, "jt");
		std::vector<std::shared_ptr<TemplateTask>> tasks = {mft, jt};
		rc = std::make_unique<RobotController>(robot, tasks);
		sim = std::make_unique<BatchedSimulation>(*rc, 0.001, 3);
		detail::check(rc->ctx(), sai2b_set_state(rc->ctx(), q.data(), dq.data(), 0));
		rc->reinitializeTasks();
		sim->setExternalWrench(6, force, Batch(), Batch(), {0.02, -0.01, 0.07}, SAI2B_WRENCH_WORLD, mft.get());
	}
	// the sensed force in the world frame: a rotation of the sensor-frame rows, the same for two rigs in the same state
	Batch sensed() const { return mft->getSensedForceControlWorldFrame(); }
};

static bool same_bits(const Batch& a, const Batch& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

static int run() {
	const int B = 130, n = 7, D = 2, periods = 6;
	const size_t sB = (size_t)B;
	sai2b_robot_model model;
	detail::check(nullptr, sai2b_panda_model(&model));
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5};
	Batch q(n * sB), dq(n * sB), force(3 * sB);
	std::vector<Batch> cmd(periods, Batch(n * sB));
	for (int b = 0; b < B; b++) {
		for (int i = 0; i < n; i++) {
			const size_t k = i * sB + b;
			q[k] = q0[i] + 0.3 * std::sin(0.37 * b + i), dq[k] = 0.2 * std::cos(0.11 * b + 2 * i);
			for (int p = 0; p < periods; p++) cmd[p][k] = 4.0 * std::sin(0.9 * p + 0.13 * b + i);
		}
		for (int a = 0; a < 3; a++) force[a * sB + b] = 10.0 * std::cos(0.2 * b + a);
	}
	// the rows: delay b mod 3, lag off, gain 1.5 on every joint, no noise; the sensor reads 2 N too much along its x
	Batch A((1 + 3 * n) * sB, 0.0), S(13 * sB, 0.0), ideal_A = A;
	for (int b = 0; b < B; b++) A[b] = b % (D + 1);
	for (size_t i = 0; i < n * sB; i++) A[sB + i] = 1.0, A[(1 + n) * sB + i] = 1.5, ideal_A[sB + i] = 1.0, ideal_A[(1 + n) * sB + i] = 1.0;
	for (int b = 0; b < B; b++) S[b] = 2.0, S[12 * sB + b] = 1.0;

	// 1: delay, gain and a sensor task through 6 periods against the known delayed command
	{
		Rig a(model, B, q, dq, force);
		a.sim->setHardware(A, S, D, a.mft.get(), 7, 0);
		bool applied_ok = true, clocks_ok = true;
		for (int p = 0; p < periods; p++) {
			a.sim->setJointTorques(cmd[p]);
			a.sim->integrate();
			const BatchedSimulation::HardwareState st = a.sim->getHardwareState();
			clocks_ok = clocks_ok && st.applied_torque.size() == n * sB && st.period.size() == sB && st.episode.size() == sB;
			for (int b = 0; b < B && clocks_ok; b++) {
				clocks_ok = st.period[b] == p + 1 && st.episode[b] == 0;
				const int past = p - b % (D + 1) > 0 ? p - b % (D + 1) : 0;
				for (int i = 0; i < n; i++) applied_ok = applied_ok && st.applied_torque[i * sB + b] == 1.5 * cmd[past][i * sB + b];
			}
		}
		check(applied_ok, "applied torque: 1.5 x the command of d periods ago, bit for bit");
		check(clocks_ok, "period and episode of every robot, sizes of the state");
		// a reset through the controller starts the next episode
		std::vector<unsigned char> mask(B, 0);
		for (int b = 0; b < B; b += 3) mask[b] = 1;
		detail::check(a.rc->ctx(), sai2b_reset_robots(a.rc->ctx(), mask.data(), nullptr, nullptr, 0));
		const BatchedSimulation::HardwareState st = a.sim->getHardwareState();
		bool reset_ok = true;
		for (int b = 0; b < B; b++) reset_ok = reset_ok && st.period[b] == (mask[b] ? 0 : periods) && st.episode[b] == (mask[b] ? 1 : 0);
		check(reset_ok, "reset: period 0 and the next episode for the selected robots");

		// the exceptions, from setHardware itself; the hardware in force stays what it was
		Rig other(model, B, q, dq, force);
		auto edited = [](Batch v, size_t i, double x) {
			v[i] = x;
			return v;
		};
		expect_invalid("actuator rows of the wrong size", [&] { a.sim->setHardware(Batch(3 * n * sB), S, D); });
		expect_invalid("sensor rows of the wrong size", [&] { a.sim->setHardware(A, Batch(12 * sB), D); });
		expect_invalid("max_delay above 8", [&] { a.sim->setHardware(Batch(), Batch(), 9); });
		expect_invalid("max_delay below 0", [&] { a.sim->setHardware(Batch(), Batch(), -1); });
		expect_invalid("delay above max_delay", [&] { a.sim->setHardware(A, S, 1); });
		expect_invalid("delay not an integer", [&] { a.sim->setHardware(edited(A, 0, 0.5), S, D); });
		expect_invalid("alpha 0", [&] { a.sim->setHardware(edited(A, sB + 3, 0.0), S, D); });
		expect_invalid("negative gain", [&] { a.sim->setHardware(edited(A, (1 + n) * sB + 1, -0.5), S, D); });
		expect_invalid("NaN sigma", [&] { a.sim->setHardware(edited(A, (1 + 2 * n) * sB, NAN), S, D); });
		expect_invalid("infinite bias", [&] { a.sim->setHardware(A, edited(S, 4, INFINITY), D); });
		expect_invalid("negative sensor noise", [&] { a.sim->setHardware(A, edited(S, 6 * sB + 2, -1.0), D); });
		expect_invalid("alpha_s above 1", [&] { a.sim->setHardware(A, edited(S, 12 * sB + 1, 1.2), D); });
		expect_invalid("sensor task of another controller", [&] { a.sim->setHardware(A, S, D, other.mft.get()); });
		sai2b_hardware_config now;
		detail::check(a.rc->ctx(), sai2b_get_hardware(a.rc->ctx(), &now, nullptr, nullptr));
		check(now.max_delay == D && now.sensor_task == 0 && now.seed == 7, "a rejected call leaves the hardware as it was");
	}

	// 2: the sensor alone (ideal actuators, empty rows = NULL) against a twin without hardware, then clearHardware
	{
		Rig a(model, B, q, dq, force), twin(model, B, q, dq, force);
		a.sim->setHardware(Batch(), S, 0, a.mft.get(), 7, 0);
		bool state_ok = true, bias_ok = true, applied_ok = true;
		for (int p = 0; p < periods; p++) {
			for (Rig* r : {&a, &twin}) {
				r->sim->setJointTorques(cmd[p]);
				r->sim->integrate();
			}
			state_ok = state_ok && same_bits(a.sim->getJointPositions(), twin.sim->getJointPositions()) &&
					   same_bits(a.sim->getJointVelocities(), twin.sim->getJointVelocities());
			applied_ok = applied_ok && same_bits(a.sim->getHardwareState().applied_torque, cmd[p]);
			const Batch fa = a.sensed(), ft = twin.sensed();
			for (int b = 0; b < B; b++) {
				double d2 = 0;
				for (int k = 0; k < 3; k++) d2 += (fa[k * sB + b] - ft[k * sB + b]) * (fa[k * sB + b] - ft[k * sB + b]);
				bias_ok = bias_ok && std::fabs(std::sqrt(d2) - 2.0) < 1e-9;
			}
		}
		check(state_ok, "ideal actuators: the state is the twin's, bit for bit");
		check(applied_ok, "ideal actuators: the applied torque is the command, bit for bit");
		check(bias_ok, "sensor: the measured force is the twin's reading plus the 2 N bias");
		a.sim->clearHardware();
		const BatchedSimulation::HardwareState st = a.sim->getHardwareState();
		bool zero = true;
		for (int b = 0; b < B; b++) zero = zero && st.period[b] == 0 && st.episode[b] == 0;
		check(zero && sai2b_device_buffer(a.rc->ctx(), SAI2B_BUF_TAU_APPLIED, -1) == nullptr, "clearHardware: no state, no applied-torque buffer");
		bool ideal_ok = true;
		for (int p = 0; p < 3; p++) {
			for (Rig* r : {&a, &twin}) {
				r->sim->setJointTorques(cmd[p]);
				r->sim->integrate();
			}
			ideal_ok = ideal_ok && same_bits(a.sim->getJointPositions(), twin.sim->getJointPositions()) && same_bits(a.sensed(), twin.sensed());
		}
		check(ideal_ok, "clearHardware: state and sensor reading are the twin's again, bit for bit");
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
	std::printf("usage: hardware_facade_test validate|run\n");
	return 2;
}

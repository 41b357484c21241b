// The joint-sensor members of the C++ facade (include/Sai2PrimitivesBatched.h: setJointSensor, clearJointSensor, jointSensorState,
// measuredState on RobotController, BatchedSimulation and ShardedRobotController).
// `validate` needs no device: the members by signature, the struct's size, the defaults and what sai2b_validate_joint_sensor
// rejects. `run`: on 130 Pandas, a pure delay through 6 periods of integrate() against the truth recorded d periods earlier, bit
// for bit; the clocks; a reset through the controller; an offset alone (measured = truth + offset, one sum); the same members
// through RobotController; std::invalid_argument from setJointSensor itself, which leaves the sensor as it was; clearJointSensor.
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
static void validate_config(sai2b_joint_sensor_config cfg) {
	char msg[256];
	if (sai2b_validate_joint_sensor(&cfg, SAI2B_DOF, msg, sizeof(msg)) == SAI2B_INVALID_ARGUMENT) throw std::invalid_argument(msg);
}

template <class T>
static void members() {
	static_assert(std::is_same<decltype(&T::setJointSensor), void (T::*)(const sai2b_joint_sensor_config&, const Batch&)>::value, "setJointSensor");
	static_assert(std::is_same<decltype(&T::clearJointSensor), void (T::*)()>::value, "clearJointSensor");
}

static int validate() {
	members<detail::JointSensorMembers>();
	members<ShardedRobotController>();
	static_assert(std::is_base_of<detail::JointSensorMembers, RobotController>::value && std::is_base_of<detail::JointSensorMembers, BatchedSimulation>::value,
				  "RobotController and BatchedSimulation share the members");
	static_assert(std::is_same<decltype(&detail::JointSensorMembers::jointSensorState), JointSensorState (detail::JointSensorMembers::*)() const>::value &&
					  std::is_same<decltype(&detail::JointSensorMembers::measuredState), MeasuredState (detail::JointSensorMembers::*)() const>::value &&
					  std::is_same<decltype(&ShardedRobotController::jointSensorState), JointSensorState (ShardedRobotController::*)()>::value &&
					  std::is_same<decltype(&ShardedRobotController::measuredState), MeasuredState (ShardedRobotController::*)()>::value,
				  "the getters");
	check(true, "members compile");
	check(sai2b_sizeof_joint_sensor_config() == (int)sizeof(sai2b_joint_sensor_config), "size of the configuration");
	sai2b_joint_sensor_config ok;
	check(sai2b_default_joint_sensor(&ok) == SAI2B_OK && ok.max_delay == 0 && ok.velocity_mode == 0 && ok.first_robot == 0 && ok.seed == 0, "defaults");
	validate_config(ok);  // accepted
	auto with = [&](int delay, int mode) {
		sai2b_joint_sensor_config c = ok;
		c.max_delay = delay, c.velocity_mode = mode;
		return c;
	};
	validate_config(with(SAI2B_MAX_ACTUATION_DELAY, 1));
	expect_invalid("max_delay above 8", [&] { validate_config(with(9, 0)); });
	expect_invalid("max_delay below 0", [&] { validate_config(with(-1, 0)); });
	expect_invalid("velocity_mode 2", [&] { validate_config(with(0, 2)); });
	check(sai2b_set_joint_sensor(nullptr, &ok, nullptr, 0) == SAI2B_INVALID_ARGUMENT, "sai2b_set_joint_sensor(NULL ctx)");
	check(sai2b_clear_joint_sensor(nullptr) == SAI2B_INVALID_ARGUMENT, "sai2b_clear_joint_sensor(NULL ctx)");
	std::printf("%d failures\n", failures);
	return failures ? 1 : 0;
}

struct Rig {
	std::shared_ptr<BatchedRobotModel> robot;
	std::shared_ptr<MotionForceTask> mft;
	std::shared_ptr<JointTask> jt;
	std::unique_ptr<RobotController> rc;
	std::unique_ptr<BatchedSimulation> sim;
	Rig(const sai2b_robot_model& model, int B, const Batch& q, const Batch& dq) {
		robot = std::make_shared<BatchedRobotModel>(B, model, 0);
		const double fp[3] = {0.0, 0.0, 0.1};
		mft = std::make_shared<MotionForceTask>(robot, 6, fp);
		jt = std::make_shared<JointTask>(robot, "jt");
		std::vector<std::shared_ptr<TemplateTask>> tasks = {mft, jt};
		rc = std::make_unique<RobotController>(robot, tasks);
		sim = std::make_unique<BatchedSimulation>(*rc, 0.001, 3);
		detail::check(rc->ctx(), sai2b_set_state(rc->ctx(), q.data(), dq.data(), 0));
		rc->reinitializeTasks();
	}
};

static bool same_bits(const Batch& a, const Batch& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

static int run() {
	const int B = 130, n = 7, D = 2, periods = 6;
	const size_t sB = (size_t)B;
	sai2b_robot_model model;
	detail::check(nullptr, sai2b_panda_model(&model));
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5};
	Batch q(n * sB), dq(n * sB);
	std::vector<Batch> cmd(periods, Batch(n * sB));
	for (int b = 0; b < B; b++)
		for (int i = 0; i < n; i++) {
			const size_t k = i * sB + b;
			q[k] = q0[i] + 0.3 * std::sin(0.37 * b + i), dq[k] = 0.2 * std::cos(0.11 * b + 2 * i);
			for (int p = 0; p < periods; p++) cmd[p][k] = 4.0 * std::sin(0.9 * p + 0.13 * b + i);
		}
	// ideal rows, then: the delay b mod 3; or an offset per joint and robot
	Batch ideal((1 + 5 * n) * sB, 0.0);
	for (size_t i = 0; i < n * sB; i++) ideal[(1 + 4 * n) * sB + i] = 1.0;
	Batch delayed = ideal, offset = ideal;
	for (int b = 0; b < B; b++) delayed[b] = b % (D + 1);
	for (size_t i = 0; i < n * sB; i++) offset[sB + i] = 0.01 * std::sin(0.7 * (double)i);
	sai2b_joint_sensor_config cfg;
	detail::check(nullptr, sai2b_default_joint_sensor(&cfg));
	cfg.max_delay = D, cfg.seed = 7;

	// 1: a pure delay through 6 periods against the truth of d periods ago
	{
		Rig a(model, B, q, dq);
		a.sim->setJointSensor(cfg, delayed);
		std::vector<Batch> tq = {a.sim->getJointPositions()}, tdq = {a.sim->getJointVelocities()};
		check(same_bits(a.sim->measuredState().q, q) && same_bits(a.sim->measuredState().dq, dq), "seeded: the measurement is the state");
		bool delay_ok = true, clocks_ok = true, moved = false;
		for (int p = 1; p <= periods; p++) {
			a.sim->setJointTorques(cmd[p - 1]);
			a.sim->integrate();
			tq.push_back(a.sim->getJointPositions()), tdq.push_back(a.sim->getJointVelocities());
			const MeasuredState m = a.rc->measuredState();	// (through the controller: the same context)
			const JointSensorState st = a.sim->jointSensorState();
			clocks_ok = clocks_ok && st.clock.size() == sB && st.episode.size() == sB && m.q.size() == n * sB && m.dq.size() == n * sB;
			for (int b = 0; b < B && clocks_ok; b++) {
				clocks_ok = st.clock[b] == p + 1 && st.episode[b] == 0;
				const int past = p - b % (D + 1) > 0 ? p - b % (D + 1) : 0;
				for (int i = 0; i < n; i++)
					delay_ok = delay_ok && m.q[i * sB + b] == tq[past][i * sB + b] && m.dq[i * sB + b] == tdq[past][i * sB + b];
			}
			moved = moved || !same_bits(tq[p], tq[p - 1]);
		}
		check(delay_ok && moved, "measured pair: the truth of d periods ago, bit for bit");
		check(clocks_ok, "clock and episode of every robot, sizes of the state");
		std::vector<unsigned char> mask(B, 0);
		for (int b = 0; b < B; b += 3) mask[b] = 1;
		a.rc->resetRobots(mask, q, dq);
		const JointSensorState st = a.rc->jointSensorState();
		const MeasuredState m = a.sim->measuredState();
		bool reset_ok = true;
		for (int b = 0; b < B; b++) {
			reset_ok = reset_ok && st.clock[b] == (mask[b] ? 1 : periods + 1) && st.episode[b] == (mask[b] ? 1 : 0);
			for (int i = 0; i < n && mask[b]; i++) reset_ok = reset_ok && m.q[i * sB + b] == q[i * sB + b] && m.dq[i * sB + b] == dq[i * sB + b];
		}
		check(reset_ok, "reset: reading 0 of the next episode for the selected robots");

		// the exceptions, from setJointSensor itself; the sensor in force stays what it was
		auto edited = [](Batch v, size_t i, double x) {
			v[i] = x;
			return v;
		};
		auto with = [&](int delay, int mode) {
			sai2b_joint_sensor_config c = cfg;
			c.max_delay = delay, c.velocity_mode = mode;
			return c;
		};
		expect_invalid("rows of the wrong size", [&] { a.sim->setJointSensor(cfg, Batch(5 * n * sB)); });
		expect_invalid("max_delay above 8", [&] { a.rc->setJointSensor(with(9, 0)); });
		expect_invalid("velocity_mode 3", [&] { a.sim->setJointSensor(with(D, 3)); });
		expect_invalid("delay above max_delay", [&] { a.sim->setJointSensor(with(1, 0), delayed); });
		expect_invalid("delay not an integer", [&] { a.sim->setJointSensor(cfg, edited(delayed, 0, 0.5)); });
		expect_invalid("infinite offset", [&] { a.sim->setJointSensor(cfg, edited(delayed, sB + 3, INFINITY)); });
		expect_invalid("negative position noise", [&] { a.sim->setJointSensor(cfg, edited(delayed, (1 + n) * sB + 1, -1e-3)); });
		expect_invalid("NaN quantum", [&] { a.sim->setJointSensor(cfg, edited(delayed, (1 + 2 * n) * sB, NAN)); });
		expect_invalid("negative velocity noise", [&] { a.sim->setJointSensor(cfg, edited(delayed, (1 + 3 * n) * sB + 2, -1.0)); });
		expect_invalid("alpha 0", [&] { a.sim->setJointSensor(cfg, edited(delayed, (1 + 4 * n) * sB + 1, 0.0)); });
		sai2b_joint_sensor_config now;
		detail::check(a.rc->ctx(), sai2b_get_joint_sensor(a.rc->ctx(), &now, nullptr));
		const JointSensorState after = a.sim->jointSensorState();
		check(now.max_delay == D && now.seed == 7 && after.clock == st.clock && after.episode == st.episode, "a rejected call leaves the sensor as it was");
	}

	// 2: an offset alone through the controller's members, the tick reads it; then clearJointSensor
	{
		Rig a(model, B, q, dq), twin(model, B, q, dq);
		sai2b_joint_sensor_config c0 = cfg;
		c0.max_delay = 0;
		a.rc->setJointSensor(c0, offset);
		bool offset_ok = true, truth_ok = true, tick_differs = false;
		for (int p = 0; p < 3; p++) {
			const Batch ta = a.rc->computeControlTorques(), tt = twin.rc->computeControlTorques();
			tick_differs = tick_differs || !same_bits(ta, tt);
			for (Rig* r : {&a, &twin}) {
				r->sim->setJointTorques(cmd[p]);
				r->sim->integrate();
			}
			truth_ok = truth_ok && same_bits(a.sim->getJointPositions(), twin.sim->getJointPositions());
			const MeasuredState m = a.sim->measuredState();
			const Batch t = a.sim->getJointPositions();
			for (size_t i = 0; i < n * sB; i++) offset_ok = offset_ok && m.q[i] == t[i] + offset[sB + i];
			offset_ok = offset_ok && same_bits(m.dq, a.sim->getJointVelocities());
		}
		check(offset_ok, "offset: measured q = truth + offset, measured dq = truth, bit for bit");
		check(truth_ok, "the plant integrates the truth: the state under the same torques is the twin's, bit for bit");
		check(tick_differs, "the controller reads the measured view: its torques are not the twin's");
		a.rc->clearJointSensor();
		const JointSensorState st = a.sim->jointSensorState();
		bool zero = true;
		for (int b = 0; b < B; b++) zero = zero && st.clock[b] == 0 && st.episode[b] == 0;
		check(zero && sai2b_device_buffer(a.rc->ctx(), SAI2B_BUF_Q_MEASURED, -1) == nullptr, "clearJointSensor: no clocks, no measured buffer");
		check(same_bits(a.sim->measuredState().q, a.sim->getJointPositions()), "clearJointSensor: one view, the truth");
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
	std::printf("usage: joint_sensor_facade_test validate|run\n");
	return 2;
}

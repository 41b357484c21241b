// Per-robot payloads through ShardedRobotController: two shards on device 0, an uneven split, against one context of the
// whole batch through the C ABI: torques bit for bit, before and after the payload is cleared. Prints "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "Sai2PrimitivesBatched.h"

using namespace Sai2Primitives;

static Batch tick_one(const sai2b_robot_model& model, const std::vector<sai2b_task_config>& cfgs, int B, const Batch& q, const Batch& dq,
					  const Batch* mass, const Batch* com, const Batch* inertia) {
	sai2b_ctx* c = sai2b_create(&model, cfgs.data(), (int)cfgs.size(), B, 0);
	if (!c) throw std::runtime_error(sai2b_last_error(nullptr));
	detail::check(c, sai2b_set_state(c, q.data(), dq.data(), 0));
	detail::check(c, sai2b_reinitialize(c));
	detail::check(c, sai2b_enable_gravity_compensation(c, 1));
	if (mass) detail::check(c, sai2b_set_link_payload(c, SAI2B_PAYLOAD_BOTH, 6, mass->data(), com->data(), inertia->data(), 0));
	Batch tau(7 * (size_t)B);
	detail::check(c, sai2b_tick(c, tau.data(), 0));
	sai2b_destroy(c);
	return tau;
}

int main() {
	const int B = 4099;
	sai2b_robot_model model;
	detail::check(nullptr, sai2b_panda_model(&model));
	std::vector<sai2b_task_config> cfgs(2);
	const double fp[3] = {0, 0, 0.1};
	detail::check(nullptr, sai2b_default_motion_force_task(&cfgs[0], "mft", 6, fp, nullptr, -1, nullptr, -1, nullptr));
	detail::check(nullptr, sai2b_default_joint_task(&cfgs[1], "jt", 7, nullptr));
	cfgs[0].use_internal_otg = cfgs[1].use_internal_otg = 0;
	const double q0[7] = {0.3, -0.4, 0.2, -1.9, 0.1, 1.6, 0.5};
	Batch q(7 * (size_t)B), dq(7 * (size_t)B), mass(B), com(3 * (size_t)B), inertia(6 * (size_t)B, 0.0);
	for (int b = 0; b < B; b++) {
		for (int i = 0; i < 7; i++) q[i * (size_t)B + b] = q0[i] + 0.3 * std::sin(0.37 * b + i), dq[i * (size_t)B + b] = 0.2 * std::cos(0.11 * b + 2 * i);
		mass[b] = 0.2 * (b % 16);
		for (int k = 0; k < 3; k++) com[k * (size_t)B + b] = 0.01 * ((b + 3 * k) % 11) - 0.05;
		for (int k = 0; k < 3; k++) inertia[k * (size_t)B + b] = 1e-3 * (1 + (b + k) % 7);
		inertia[3 * (size_t)B + b] = 2e-4 * ((b % 5) - 2);
	}
	ShardedRobotController sharded(model, cfgs, B, {0, 0});
	if (sharded.shardBounds(0).second - sharded.shardBounds(0).first == sharded.shardBounds(1).second - sharded.shardBounds(1).first) return 2;
	sharded.setState(q, dq);
	sharded.reinitializeTasks();
	sharded.enableGravityCompensation(true);
	sharded.setLinkPayload(6, mass, com, inertia);
	const Batch with = sharded.tick(), with_ref = tick_one(model, cfgs, B, q, dq, &mass, &com, &inertia);
	sharded.clearLinkPayload();
	const Batch without = sharded.tick(), without_ref = tick_one(model, cfgs, B, q, dq, nullptr, nullptr, nullptr);
	if (std::memcmp(with.data(), with_ref.data(), with.size() * sizeof(double)) != 0) return 3;
	if (std::memcmp(without.data(), without_ref.data(), without.size() * sizeof(double)) != 0) return 4;
	if (std::memcmp(with.data(), without.data(), with.size() * sizeof(double)) == 0) return 5;
	std::printf("ok\n");
	return 0;
}

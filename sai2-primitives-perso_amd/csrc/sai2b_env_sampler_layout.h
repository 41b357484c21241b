// sai2b_env_sampler_layout.h — the sample rows of the environment sampler (include/sai2b.h "environment sampler"), the rows of
// its nominal buffer, what the host checks of its configuration and the configuration as the draws read it, decided from the
// configuration and the joint count alone. No HIP in here: sai2b_host.cpp uses it for the context,
// tests/cpp/env_sampler_driver.cpp runs it on a CPU.
// (The functions are static: every per-size build has its own, and the library exports none of them.)
#pragma once
#include <cmath>
#include <string>

#include "../../include/sai2b.h"
#include "sai2b_env_draw.h"

namespace sai2b {

constexpr int ENV_GROUPS = 5;
constexpr unsigned ENV_ALL_GROUPS = SAI2B_ENV_PAYLOAD | SAI2B_ENV_CONTACT | SAI2B_ENV_JOINT_DYNAMICS | SAI2B_ENV_HARDWARE | SAI2B_ENV_PUSH;

// first sample row of group g (bit 1 << g) and its rows; -1 / 0 for a group the configuration does not hold
struct EnvLayout {
	int total = 0;
	int first[ENV_GROUPS] = {-1, -1, -1, -1, -1};
	int rows[ENV_GROUPS] = {0, 0, 0, 0, 0};
};

static inline int env_group_rows(int g, int dof) {
	switch (g) {
		case 0: return ENV_PAYLOAD_ROWS;
		case 1: return ENV_CONTACT_ROWS;
		case 2: return ENV_JOINT_PARAMS * dof;
		case 3: return ENV_HW_FIXED_ROWS + ENV_HW_PARAMS * dof;
		default: return ENV_PUSH_ROWS;
	}
}

static inline EnvLayout env_layout(unsigned groups, int dof) {
	EnvLayout L;
	for (int g = 0; g < ENV_GROUPS; g++) {
		if (!(groups >> g & 1u)) continue;
		L.first[g] = L.total, L.rows[g] = env_group_rows(g, dof);
		L.total += L.rows[g];
	}
	return L;
}

// rows of the nominal buffer, every group at a fixed place: plant payload 10, controller payload 10, contact 9, joint dynamics
// 4 dof, actuator 1 + 3 dof, sensor 12
struct EnvNominal {
	int plant_payload, payload, contact, joint, actuator, sensor, total;
};
static inline EnvNominal env_nominal(int dof) {
	EnvNominal n;
	n.plant_payload = 0, n.payload = 10, n.contact = 20, n.joint = 29;
	n.actuator = n.joint + ENV_JOINT_PARAMS * dof, n.sensor = n.actuator + 1 + ENV_HW_PARAMS * dof, n.total = n.sensor + 12;
	return n;
}

static inline std::string env_range_error(const sai2b_env_range& r, const char* name, bool scale, bool positive = false) {
	const std::string n = std::string("env sampler: ") + name;
	if (!std::isfinite(r.lower) || !std::isfinite(r.upper)) return n + " must be finite";
	if (r.lower > r.upper) return n + ": lower must not exceed upper";
	if (r.log_uniform != 0 && r.log_uniform != 1) return n + ": log_uniform must be 0 or 1";
	if (scale && r.lower < 0) return n + ": lower must not be negative";
	if (r.log_uniform && r.lower <= 0) return n + ": a log-uniform range needs lower > 0";
	if (positive && !(r.lower > 0)) return n + ": lower must be > 0";
	return "";
}

// "" or the reason the configuration is rejected
static inline std::string env_config_error(const sai2b_env_sampler_config* c) {
	if (!c) return "env sampler: null config";
	if (c->groups & ~ENV_ALL_GROUPS) return "env sampler: groups holds a bit that is no group";
	if (c->payload_target != SAI2B_PAYLOAD_PLANT && c->payload_target != SAI2B_PAYLOAD_BOTH)
		return "env sampler: payload_target must be SAI2B_PAYLOAD_PLANT or SAI2B_PAYLOAD_BOTH";
	struct {
		const sai2b_env_range* r;
		const char* name;
		bool scale, positive;
	} const ranges[] = {{&c->payload_mass_scale, "payload_mass_scale", true, false},
						{&c->contact_height, "contact_height", false, false},
						{&c->contact_stiffness_scale, "contact_stiffness_scale", true, false},
						{&c->contact_damping_scale, "contact_damping_scale", true, false},
						{&c->contact_friction_scale, "contact_friction_scale", true, false},
						{&c->armature_scale, "armature_scale", true, false},
						{&c->damping_scale, "damping_scale", true, false},
						{&c->friction_scale, "friction_scale", true, false},
						{&c->torque_limit_scale, "torque_limit_scale", true, false},
						{&c->lag_scale, "lag_scale", true, true},
						{&c->gain_scale, "gain_scale", true, false},
						{&c->torque_noise_scale, "torque_noise_scale", true, false},
						{&c->sensor_noise_scale, "sensor_noise_scale", true, false},
						{&c->push_force, "push_force", true, false},
						{&c->push_moment, "push_moment", true, false}};
	for (const auto& e : ranges) {
		const std::string err = env_range_error(*e.r, e.name, e.scale, e.positive);
		if (!err.empty()) return err;
	}
	for (int k = 0; k < 3; k++)
		if (!(c->payload_com_half[k] >= 0) || !std::isfinite(c->payload_com_half[k]))
			return "env sampler: payload_com_half must be finite and not negative";
	for (int k = 0; k < 6; k++)
		if (!(c->sensor_bias_half[k] >= 0) || !std::isfinite(c->sensor_bias_half[k]))
			return "env sampler: sensor_bias_half must be finite and not negative";
	if (!(c->contact_tilt_max >= 0 && c->contact_tilt_max <= 3.141592653589793)) return "env sampler: contact_tilt_max must be in [0, pi]";
	if (c->delay_lower < 0 || c->delay_upper > SAI2B_MAX_ACTUATION_DELAY) return "env sampler: the delay must lie in [0, SAI2B_MAX_ACTUATION_DELAY]";
	if (c->delay_lower > c->delay_upper) return "env sampler: delay_lower must not exceed delay_upper";
	if (c->push_steps_lower < 0) return "env sampler: push steps must not be negative";
	if (c->push_steps_lower > c->push_steps_upper) return "env sampler: push_steps_lower must not exceed push_steps_upper";
	return "";
}

static inline void env_default_config(sai2b_env_sampler_config* c) {
	*c = sai2b_env_sampler_config{};
	c->payload_target = SAI2B_PAYLOAD_PLANT;
	sai2b_env_range* const scales[] = {&c->payload_mass_scale, &c->contact_stiffness_scale, &c->contact_damping_scale, &c->contact_friction_scale,
									   &c->armature_scale,	   &c->damping_scale,			&c->friction_scale,		   &c->torque_limit_scale,
									   &c->lag_scale,		   &c->gain_scale,				&c->torque_noise_scale,	   &c->sensor_noise_scale};
	for (sai2b_env_range* r : scales) r->lower = r->upper = 1.0;
}

static inline EnvRange env_range_params(const sai2b_env_range& r) {
	EnvRange e;
	if (r.log_uniform) {
		const double la = std::log(r.lower), lb = std::log(r.upper);
		e.a = la, e.w = lb - la, e.log = 1;
	} else
		e.a = r.lower, e.w = r.upper - r.lower, e.log = 0;
	return e;
}

// the configuration as the draws read it
static inline EnvDraw env_draw_params(const sai2b_env_sampler_config& c) {
	EnvDraw d;
	d.payload_mass = env_range_params(c.payload_mass_scale);
	for (int k = 0; k < 3; k++) d.payload_com_half[k] = c.payload_com_half[k];
	d.contact_height = env_range_params(c.contact_height);
	d.contact_scale[0] = env_range_params(c.contact_stiffness_scale);
	d.contact_scale[1] = env_range_params(c.contact_damping_scale);
	d.contact_scale[2] = env_range_params(c.contact_friction_scale);
	d.contact_tilt_max = c.contact_tilt_max;
	d.joint_scale[0] = env_range_params(c.armature_scale), d.joint_scale[1] = env_range_params(c.damping_scale);
	d.joint_scale[2] = env_range_params(c.friction_scale), d.joint_scale[3] = env_range_params(c.torque_limit_scale);
	d.hw_scale[0] = env_range_params(c.lag_scale), d.hw_scale[1] = env_range_params(c.gain_scale);
	d.hw_scale[2] = env_range_params(c.torque_noise_scale);
	d.sensor_noise = env_range_params(c.sensor_noise_scale);
	for (int k = 0; k < 6; k++) d.sensor_bias_half[k] = c.sensor_bias_half[k];
	d.push_force = env_range_params(c.push_force), d.push_moment = env_range_params(c.push_moment);
	d.delay_lower = c.delay_lower, d.delay_upper = c.delay_upper;
	d.steps_lower = c.push_steps_lower, d.steps_upper = c.push_steps_upper;
	return d;
}

}  // namespace sai2b

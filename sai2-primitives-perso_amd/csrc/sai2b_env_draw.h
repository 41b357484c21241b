// sai2b_env_draw.h — what the environment sampler (include/sai2b.h "environment sampler") draws from the generator of
// sai2b_rng.h: per group, a pure function of (draw counter, robot, key, the batch-uniform ranges, the robot's nominal rows) that
// gives the robot's new rows and the drawn quantities themselves (the sample rows). env_randomize_kernel
// (sai2b_env_sampler.hip) and a CPU program (tests/cpp/env_sampler_driver.cpp) run the same code. No HIP in here when a host
// compiler reads it.
// Affine maps and products are one product and one sum, never a fused multiply-add: clang is told so below; a GCC build passes
// -ffp-contract=off (the library's translation unit does too).
#pragma once
#include "sai2b_reset_draw.h"

namespace sai2b {

enum { ENV_STREAM_PAYLOAD = 5, ENV_STREAM_CONTACT = 6, ENV_STREAM_JOINT = 7, ENV_STREAM_HARDWARE = 8, ENV_STREAM_PUSH = 9 };
// rows of a group in the sample buffer (joint dynamics: 4 dof; hardware: ENV_HW_FIXED_ROWS + 3 dof)
constexpr int ENV_PAYLOAD_ROWS = 4, ENV_CONTACT_ROWS = 8, ENV_PUSH_ROWS = 9, ENV_HW_FIXED_ROWS = 8, ENV_JOINT_PARAMS = 4, ENV_HW_PARAMS = 3;

// a range as the device takes it: s = a + w u, or exp(a + w u) with the logarithms taken on the host
struct EnvRange {
	double a = 1, w = 0;
	int log = 0, pad = 0;
};
// the batch-uniform part of sai2b_env_sampler_config as the draws read it (sai2b_env_sampler_layout.h: env_draw_params)
struct EnvDraw {
	EnvRange payload_mass;
	double payload_com_half[3] = {0, 0, 0};
	EnvRange contact_height, contact_scale[3];	// stiffness, damping, friction
	double contact_tilt_max = 0;
	EnvRange joint_scale[ENV_JOINT_PARAMS];	 // armature, damping, friction, torque limit
	EnvRange hw_scale[ENV_HW_PARAMS];		 // lag, gain, torque noise
	EnvRange sensor_noise;
	double sensor_bias_half[6] = {0, 0, 0, 0, 0, 0};
	EnvRange push_force, push_moment;
	int delay_lower = 0, delay_upper = 0, steps_lower = 0, steps_upper = 0;
};

// the four uniforms of call `call` of stream `stream` for draw counter c: counter (0, c, 256 stream + call, robot)
SAI2B_RNG_HD inline void env_uniforms4(unsigned c, unsigned stream, unsigned call, unsigned robot, unsigned k0, unsigned k1, double u[4]) {
	rs_uniforms4(0u, c, stream, call, robot, k0, k1, u);
}

SAI2B_RNG_HD inline double env_range(const EnvRange& r, double u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double p = r.w * u;
	const double s = r.a + p;
	return r.log ? exp(s) : s;
}

// lo + min((int) floor((hi - lo + 1) u), hi - lo), as a double
SAI2B_RNG_HD inline double env_int(int lo, int hi, double u) {
	const int span = hi - lo;
	int k = (int)floor((double)(span + 1) * u);
	if (k > span) k = span;
	return (double)(lo + k);
}

SAI2B_RNG_HD inline double env_mul(double nominal, double s) { return nominal * s; }

// the direction (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z), z = 2 u0 - 1, phi = 2 pi u1, as rs_axis_rotation has its axis
SAI2B_RNG_HD inline void env_direction(double u0, double u1, double a[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double c = 2.0 * u0 - 1.0, phi = 6.283185307179586 * u1;
	const double r = sqrt(1.0 - c * c);
	a[0] = r * cos(phi), a[1] = r * sin(phi), a[2] = c;
}

// PAYLOAD. nominal / out: [10] = mass, com 3, inertia 6; sample [4] = s, o 3. The same sample serves a second target:
// env_payload_apply with that target's nominal.
SAI2B_RNG_HD inline void env_payload_sample(const EnvDraw& D, unsigned c, unsigned robot, unsigned k0, unsigned k1, double sample[4]) {
	double u[4];
	env_uniforms4(c, ENV_STREAM_PAYLOAD, 0u, robot, k0, k1, u);
	sample[0] = env_range(D.payload_mass, u[0]);
	for (int k = 0; k < 3; k++) sample[1 + k] = rs_joint_offset(D.payload_com_half[k], u[1 + k]);
}
SAI2B_RNG_HD inline void env_payload_apply(const double sample[4], const double nominal[10], double out[10]) {
	out[0] = env_mul(nominal[0], sample[0]);
	for (int k = 0; k < 3; k++) out[1 + k] = nominal[1 + k] + sample[1 + k];
	for (int k = 0; k < 6; k++) out[4 + k] = env_mul(nominal[4 + k], sample[0]);
}

// CONTACT. nominal / out: [9] = plane point 3, normal 3, stiffness, damping, friction; sample [8] = h, theta, axis 3, scales 3
SAI2B_RNG_HD inline void env_contact(const EnvDraw& D, unsigned c, unsigned robot, unsigned k0, unsigned k1, const double nominal[9], double out[9],
									 double sample[8]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	double u[4], v[4];
	env_uniforms4(c, ENV_STREAM_CONTACT, 0u, robot, k0, k1, u);
	env_uniforms4(c, ENV_STREAM_CONTACT, 1u, robot, k0, k1, v);
	const double h = env_range(D.contact_height, u[0]);
	const double theta = D.contact_tilt_max * u[1];
	double R[9];
	rs_axis_rotation(theta, u[2], u[3], sample + 2, R);
	sample[0] = h, sample[1] = theta;
	const double* n = nominal + 3;
	for (int k = 0; k < 3; k++) {
		const double hn = h * n[k];
		out[k] = nominal[k] + hn;
		const double x = R[3 * k] * n[0], y = R[3 * k + 1] * n[1], z = R[3 * k + 2] * n[2];
		out[3 + k] = theta != 0.0 ? (x + y) + z : n[k];
	}
	for (int k = 0; k < 3; k++) {
		sample[5 + k] = env_range(D.contact_scale[k], v[k]);
		out[6 + k] = env_mul(nominal[6 + k], sample[5 + k]);
	}
}

// four per-joint scales of one range: the words of one call
SAI2B_RNG_HD inline void env_scales4(const EnvRange& r, unsigned c, unsigned stream, unsigned call, unsigned robot, unsigned k0, unsigned k1,
									 double s[4]) {
	double u[4];
	env_uniforms4(c, stream, call, robot, k0, k1, u);
	for (int i = 0; i < 4; i++) s[i] = env_range(r, u[i]);
}
// JOINT DYNAMICS, parameter p (0 armature, 1 damping, 2 friction, 3 torque limit), joints 4 j .. 4 j + 3: call 2 p + j
SAI2B_RNG_HD inline void env_joint4(const EnvDraw& D, int p, int j, unsigned c, unsigned robot, unsigned k0, unsigned k1, const double nominal[4],
									double out[4], double sample[4]) {
	env_scales4(D.joint_scale[p], c, ENV_STREAM_JOINT, (unsigned)(2 * p + j), robot, k0, k1, sample);
	for (int i = 0; i < 4; i++) out[i] = env_mul(nominal[i], sample[i]);
}
// HARDWARE, parameter p (0 lag, 1 gain, 2 torque noise), joints 4 j .. 4 j + 3: call 1 + 2 p + j. The lag is clipped at 1;
// returns a bit mask of the joints (of these four) whose lag was clipped
SAI2B_RNG_HD inline int env_hardware4(const EnvDraw& D, int p, int j, unsigned c, unsigned robot, unsigned k0, unsigned k1, const double nominal[4],
									  double out[4], double sample[4]) {
	env_scales4(D.hw_scale[p], c, ENV_STREAM_HARDWARE, (unsigned)(1 + 2 * p + j), robot, k0, k1, sample);
	int clipped = 0;
	for (int i = 0; i < 4; i++) {
		double v = env_mul(nominal[i], sample[i]);
		if (p == 0 && v > 1.0) v = 1.0, clipped |= 1 << i;
		out[i] = v;
	}
	return clipped;
}
// the delay: call 0 word 0
SAI2B_RNG_HD inline double env_delay(const EnvDraw& D, unsigned c, unsigned robot, unsigned k0, unsigned k1) {
	double u[4];
	env_uniforms4(c, ENV_STREAM_HARDWARE, 0u, robot, k0, k1, u);
	return env_int(D.delay_lower, D.delay_upper, u[0]);
}
// the sensor: nominal / out [12] = bias 6, noise deviation 6; sample [7] = the six bias offsets, the noise scale
SAI2B_RNG_HD inline void env_sensor(const EnvDraw& D, unsigned c, unsigned robot, unsigned k0, unsigned k1, const double nominal[12], double out[12],
									double sample[7]) {
	double u[8];
	env_uniforms4(c, ENV_STREAM_HARDWARE, 7u, robot, k0, k1, u);
	env_uniforms4(c, ENV_STREAM_HARDWARE, 8u, robot, k0, k1, u + 4);
	for (int k = 0; k < 6; k++) {
		sample[k] = rs_joint_offset(D.sensor_bias_half[k], u[k]);
		out[k] = nominal[k] + sample[k];
	}
	sample[6] = env_range(D.sensor_noise, u[6]);
	for (int k = 0; k < 6; k++) out[6 + k] = env_mul(nominal[6 + k], sample[6]);
}

// PUSH. out [7] = force 3, moment 3, steps; sample [9] = force magnitude, direction 3, steps, moment magnitude, direction 3
SAI2B_RNG_HD inline void env_push(const EnvDraw& D, unsigned c, unsigned robot, unsigned k0, unsigned k1, double out[7], double sample[9]) {
	double u[4], v[4];
	env_uniforms4(c, ENV_STREAM_PUSH, 0u, robot, k0, k1, u);
	env_uniforms4(c, ENV_STREAM_PUSH, 1u, robot, k0, k1, v);
	sample[0] = env_range(D.push_force, u[0]);
	env_direction(u[1], u[2], sample + 1);
	sample[4] = env_int(D.steps_lower, D.steps_upper, u[3]);
	sample[5] = env_range(D.push_moment, v[0]);
	env_direction(v[1], v[2], sample + 6);
	for (int k = 0; k < 3; k++) out[k] = env_mul(sample[0], sample[1 + k]), out[3 + k] = env_mul(sample[5], sample[6 + k]);
	out[6] = sample[4];
}

}  // namespace sai2b

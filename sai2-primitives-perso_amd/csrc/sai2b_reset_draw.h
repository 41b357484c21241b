// sai2b_reset_draw.h — what the episode sampler (include/sai2b.h "episode starts") draws from the generator of sai2b_rng.h:
// a candidate joint vector inside a box, a velocity, a goal offset, a goal rotation about a uniformly drawn axis and a joint
// goal. Each is a pure function of (counter, key, the robot's rows), so reset_sampled_kernel (sai2b_otg.hip) and a CPU program
// (tests/cpp/reset_sampler_driver.cpp) run the same code. No HIP in here when a host compiler reads it.
// The affine maps are one product and one sum, never a fused multiply-add: clang is told so below; a GCC build passes
// -ffp-contract=off (the library's translation unit does too).
#pragma once
#include "sai2b_rng.h"

namespace sai2b {

enum { RS_STREAM_CANDIDATE = 2, RS_STREAM_VELOCITY = 3, RS_STREAM_GOAL = 4 };  // streams 0 and 1 are the hardware's

// u = (x + 0.5) 2^-32: in (0, 1) for every word, exact in a double
SAI2B_RNG_HD inline double rs_uniform(unsigned x) { return ((double)x + 0.5) * 2.3283064365386963e-10; }

// lower + (upper - lower) u: lower == upper gives lower exactly
SAI2B_RNG_HD inline double rs_lerp(double lower, double upper, double u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double w = upper - lower;
	const double s = w * u;
	return lower + s;
}

// the four uniforms of call `call` of stream `stream`: counter (n, e, 256 stream + call, robot)
SAI2B_RNG_HD inline void rs_uniforms4(unsigned n, unsigned e, unsigned stream, unsigned call, unsigned robot, unsigned k0, unsigned k1, double u[4]) {
	unsigned x[4] = {n, e, 256u * stream + call, robot};
	philox4x32_10(x, k0, k1);
	for (int i = 0; i < 4; i++) u[i] = rs_uniform(x[i]);
}

// candidate n of episode e: joints 4 call .. 4 call + 3 (those below dof) from call `call`
SAI2B_RNG_HD inline void rs_candidate4(unsigned n, unsigned e, unsigned call, unsigned robot, unsigned k0, unsigned k1, const double lower[4],
									   const double upper[4], double q[4]) {
	double u[4];
	rs_uniforms4(n, e, RS_STREAM_CANDIDATE, call, robot, k0, k1, u);
	for (int i = 0; i < 4; i++) q[i] = rs_lerp(lower[i], upper[i], u[i]);
}

// dq_i = sigma_i z_i of call `call`; sigma == 0 gives exactly 0
SAI2B_RNG_HD inline void rs_velocity4(unsigned e, unsigned call, unsigned robot, unsigned k0, unsigned k1, const double sigma[4], double dq[4]) {
	double z[4];
	normals4(0u, e, RS_STREAM_VELOCITY, call, robot, k0, k1, z);
	for (int i = 0; i < 4; i++) dq[i] = sigma[i] != 0.0 ? sigma[i] * z[i] : 0.0;
}

// the rotation about the axis (sqrt(1 - c^2) cos phi, sqrt(1 - c^2) sin phi, c), c = 2 u0 - 1, phi = 2 pi u1, by theta:
// D = I + sin(theta) K + (1 - cos(theta)) K^2, row-major
SAI2B_RNG_HD inline void rs_axis_rotation(double theta, double u0, double u1, double axis[3], double D[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double c = 2.0 * u0 - 1.0, phi = 6.283185307179586 * u1;
	const double r = sqrt(1.0 - c * c);
	axis[0] = r * cos(phi), axis[1] = r * sin(phi), axis[2] = c;
	const double s = sin(theta), v = 1.0 - cos(theta);
	const double x = axis[0], y = axis[1], z = axis[2];
	// K = [[0, -z, y], [z, 0, -x], [-y, x, 0]];  K^2 = a a^T - |a|^2 I, written out with |a|^2 as the sum of the squares
	const double xx = x * x, yy = y * y, zz = z * z;
	D[0] = 1.0 - v * (yy + zz), D[1] = v * (x * y) - s * z, D[2] = v * (x * z) + s * y;
	D[3] = v * (x * y) + s * z, D[4] = 1.0 - v * (xx + zz), D[5] = v * (y * z) - s * x;
	D[6] = v * (x * z) - s * y, D[7] = v * (y * z) + s * x, D[8] = 1.0 - v * (xx + yy);
}

// goal rotation = R D (row-major 3 x 3), each element a sum of three products from the left
SAI2B_RNG_HD inline void rs_rotate(const double R[9], const double D[9], double out[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) {
			const double a = R[3 * i] * D[j], b = R[3 * i + 1] * D[3 + j], c = R[3 * i + 2] * D[6 + j];
			out[3 * i + j] = (a + b) + c;
		}
}

// JointTask goal offset: half_width (2 u - 1)
SAI2B_RNG_HD inline double rs_joint_offset(double half_width, double u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double w = 2.0 * u - 1.0;
	return half_width * w;
}

}  // namespace sai2b

// sai2b_joint_sensor_law.h — one reading of a robot's joint sensors (include/sai2b.h "joint sensors"): calibration offset,
// position noise, quantisation, the velocity estimate (tachometer or finite difference of the quantised positions, noise, a
// first-order filter) and the bus latency of the reading. A pure function of the robot's rows, its state and the generator of
// sai2b_rng.h, so joint_sense_kernel (sai2b_joint_sensor.hip) and a CPU program (tests/cpp/joint_sensor_driver.cpp) run the
// same code. No HIP in here when a host compiler reads it.
// Every buffer is [row][stride]: the kernel passes its column (base + b) with stride B, the CPU program a robot of its own with
// stride 1. The sums are one product and one sum, never a fused multiply-add: clang is told so below; a GCC build passes
// -ffp-contract=off.
#pragma once
#include <cstddef>

#include "sai2b_rng.h"

namespace sai2b {

enum { JS_STREAM = 10 };  // streams 0-9 are the hardware's, the episode sampler's and the environment sampler's
enum { JS_TACHOMETER = 0, JS_FINITE_DIFFERENCE = 1 };

constexpr int js_rows(int dof) { return 1 + 5 * dof; }	// delay; offset, position noise, quantum, velocity noise, filter coefficient
constexpr int js_calls(int dof) { return (2 * dof + 3) / 4; }

// this robot draws: one of its two deviation rows is not zero
template <int DOF>
SAI2B_RNG_HD inline bool joint_sensor_noisy(const double* R, size_t sB) {
	bool noisy = false;
	for (int i = 0; i < DOF; i++) noisy = noisy || R[(size_t)(1 + DOF + i) * sB] != 0.0 || R[(size_t)(1 + 3 * DOF + i) * sB] != 0.0;
	return noisy;
}

// Reading m of episode e. R: the robot's rows; q, dq: the truth; dt: the period that produced it (not read at m == 0); depth: D;
// draw: the generator runs (the kernel: some lane of the wavefront is noisy); prev, filt: pprev and v [DOF]; hist:
// [(D + 1)][2 DOF] of (p, v), not touched when D == 0; q_meas, dq_meas: the delivered pair; q_pose != NULL: q_meas as it was on
// entry is saved there first.
template <int DOF>
SAI2B_RNG_HD inline void joint_sensor_reading(const double* R, size_t sB, const double* q, const double* dq, double dt, int m, int e, int mode,
											  int depth, bool draw, unsigned k0, unsigned k1, unsigned robot, double* prev, double* filt,
											  double* hist, double* q_meas, double* dq_meas, double* q_pose) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	// the rows are not inspected when a device-resident producer writes them: a NaN delay acts as 0
	const int d = (int)fmin(fmax(R[0], 0.0), (double)depth);
	constexpr int NZ = 4 * js_calls(DOF);
	double z[NZ];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int i = 0; i < NZ; i++) z[i] = 0.0;
	if (draw) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for (int j = 0; j < js_calls(DOF); j++) normals4((unsigned)m, (unsigned)e, JS_STREAM, (unsigned)j, robot, k0, k1, z + 4 * j);
	}
	double p[DOF], v[DOF];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int i = 0; i < DOF; i++) {
		const double o = R[(size_t)(1 + i) * sB], s = R[(size_t)(1 + DOF + i) * sB], quantum = R[(size_t)(1 + 2 * DOF + i) * sB];
		const double r = R[(size_t)(1 + 3 * DOF + i) * sB], alpha = R[(size_t)(1 + 4 * DOF + i) * sB];
		double x = q[(size_t)i * sB];
		if (o != 0.0) x = x + o;
		if (s != 0.0) {
			const double sz = s * z[i];
			x = x + sz;
		}
		p[i] = quantum > 0.0 ? quantum * rint(x / quantum) : x;
		double w = dq[(size_t)i * sB];
		if (mode == JS_FINITE_DIFFERENCE && m > 0) w = (p[i] - prev[(size_t)i * sB]) / dt;
		if (r != 0.0) {
			const double rz = r * z[DOF + i];
			w = w + rz;
		}
		v[i] = w;
		if (!(m == 0 || alpha == 1.0)) {
			const double v0 = filt[(size_t)i * sB];
			const double step = alpha * (w - v0);
			v[i] = v0 + step;
		}
		prev[(size_t)i * sB] = p[i];
		filt[(size_t)i * sB] = v[i];
	}
	if (q_pose) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for (int i = 0; i < DOF; i++) q_pose[(size_t)i * sB] = q_meas[(size_t)i * sB];
	}
	if (depth > 0) {
		const int past = m > d ? m - d : 0;
		double* hw = hist + (size_t)(m % (depth + 1)) * (2 * DOF) * sB;
		const double* hr = hist + (size_t)(past % (depth + 1)) * (2 * DOF) * sB;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for (int i = 0; i < DOF; i++) hw[(size_t)i * sB] = p[i], hw[(size_t)(DOF + i) * sB] = v[i];
		if (past != m) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
			for (int i = 0; i < DOF; i++) p[i] = hr[(size_t)i * sB], v[i] = hr[(size_t)(DOF + i) * sB];
		}
	}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int i = 0; i < DOF; i++) q_meas[(size_t)i * sB] = p[i], dq_meas[(size_t)i * sB] = v[i];
}

}  // namespace sai2b

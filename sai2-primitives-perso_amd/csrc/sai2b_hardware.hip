// sai2b_hardware.hip — the signal path between controller and plant (include/sai2b.h "actuator and force-sensor models"):
// actuate_kernel ahead of the simulation kernel turns the commanded torques into the applied ones (transport delay, first-order
// lag, gain error, noise), sense_kernel behind it turns the ideal wrench reading into the measured one (bias, noise, filter),
// hardware_reset_kernel restarts the selected robots' clocks. They are stages of their own, not more forms of the simulation
// kernel: every existing kernel keeps its instruction stream.
//
// One lane per robot, one wavefront per workgroup, as everywhere in this library. Every buffer is [row][B], so a wavefront's
// 64 lanes touch 512 contiguous bytes per row; the history is [slot][joint][B] and the lanes of a wavefront may read different
// slots (the delay is per robot), each still its own column. A lane reads and writes only its own column, so a kernel needs no
// synchronisation. Loops over joints are unrolled (N is a compile-time constant). No LDS.
//
// Noise: sai2b_rng.h, counter (period, episode, 256 stream + call, first_robot + b). A wavefront whose deviation rows are all
// zero does not draw; a lane whose own deviation is zero takes k f (or r + bias) as it is, so the result of a robot does not
// depend on whether its neighbours made the wavefront draw.
//
// Limits: the period counter is an int that only a reset takes back to 0; n % (D + 1) and (unsigned)n are wrong once it has
// passed 2^31 - 1 (24 days of 1 ms periods without a reset; include/sai2b.h says so). The key and first_robot come with every
// launch from the configuration in force, never from a snapshot bank.
#include <hip/hip_runtime.h>

#include "sai2b_launch.h"
#include "sai2b_rng.h"

namespace sai2b {

__global__ __launch_bounds__(64) void actuate_kernel(const ActuateParams P, const int B) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	const size_t sB = (size_t)B;
	const int n = P.clock[b], e = P.clock[sB + b];
	P.clock[b] = n + 1;
	const double* R = P.rows + b;
	// the rows are not inspected when a device-resident producer writes them: a NaN delay acts as 0
	const int D = P.depth;
	const int d = (int)fmin(fmax(R[0], 0.0), (double)D);
	double u[N], sig[N];
	bool noisy = false;
#pragma unroll
	for (int i = 0; i < N; i++) {
		u[i] = P.command[(size_t)i * sB + b];
		sig[i] = R[(size_t)(1 + 2 * N + i) * sB];
		noisy = noisy || sig[i] != 0.0;
	}
	if (D > 0) {
		const int past = n > d ? n - d : 0;
		double* hw = P.history + (size_t)(n % (D + 1)) * N * sB + b;
		const double* hr = P.history + (size_t)(past % (D + 1)) * N * sB + b;
#pragma unroll
		for (int i = 0; i < N; i++) hw[(size_t)i * sB] = u[i];
		if (past != n) {
#pragma unroll
			for (int i = 0; i < N; i++) u[i] = hr[(size_t)i * sB];
		}
	}
	double z[(N + 3) / 4 * 4];
#pragma unroll
	for (int i = 0; i < (N + 3) / 4 * 4; i++) z[i] = 0.0;
	if (__any(noisy)) {
#pragma unroll
		for (int j = 0; j < (N + 3) / 4; j++)
			normals4((unsigned)n, (unsigned)e, HW_STREAM_ACTUATOR, (unsigned)j, P.rng.first_robot + (unsigned)b, P.rng.key0, P.rng.key1, z + 4 * j);
	}
#pragma unroll
	for (int i = 0; i < N; i++) {
		const double alpha = R[(size_t)(1 + i) * sB], gain = R[(size_t)(1 + N + i) * sB];
		double* fp = P.filter + (size_t)i * sB + b;
		double f = u[i];
		if (!(n == 0 || alpha == 1.0)) {
			const double f0 = *fp;
			f = f0 + alpha * (u[i] - f0);
		}
		*fp = f;
		const double kf = gain * f;
		P.applied[(size_t)i * sB + b] = sig[i] != 0.0 ? kf + sig[i] * z[i] : kf;
	}
}

__global__ __launch_bounds__(64) void sense_kernel(const SenseParams P, const int B) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	const size_t sB = (size_t)B;
	const int n = P.clock[b] - 1, e = P.clock[sB + b];	// the period actuate_kernel served in this call
	const double* R = P.rows + b;
	double s[6];
	bool noisy = false;
#pragma unroll
	for (int k = 0; k < 6; k++) {
		s[k] = R[(size_t)(6 + k) * sB];
		noisy = noisy || s[k] != 0.0;
	}
	double z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	if (__any(noisy)) {
#pragma unroll
		for (int j = 0; j < 2; j++)
			normals4((unsigned)n, (unsigned)e, HW_STREAM_SENSOR, (unsigned)j, P.rng.first_robot + (unsigned)b, P.rng.key0, P.rng.key1, z + 4 * j);
	}
	const double alpha = R[12 * sB];
#pragma unroll
	for (int k = 0; k < 6; k++) {
		double* rp = P.sensed + (size_t)k * sB + b;
		double* gp = P.filter + (size_t)(N + k) * sB + b;
		const double biased = *rp + R[(size_t)k * sB];
		const double y = s[k] != 0.0 ? biased + s[k] * z[k] : biased;
		double g = y;
		if (!(n == 0 || alpha == 1.0)) {
			const double g0 = *gp;
			g = g0 + alpha * (y - g0);
		}
		*gp = g;
		*rp = g;
	}
}

__global__ __launch_bounds__(64) void hardware_reset_kernel(const unsigned char* mask, int* clock, const int B) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B || mask[b] == 0) return;
	clock[b] = 0;
	clock[(size_t)B + b] += 1;
}

int launch_actuate(int B, const ActuateParams& p, hipStream_t stream) {
	hipLaunchKernelGGL(actuate_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, p, B);
	return launch_result();
}

int launch_sense(int B, const SenseParams& p, hipStream_t stream) {
	hipLaunchKernelGGL(sense_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, p, B);
	return launch_result();
}

int launch_hardware_reset(int B, const unsigned char* mask, int* clock, hipStream_t stream) {
	hipLaunchKernelGGL(hardware_reset_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, mask, clock, B);
	return launch_result();
}

}  // namespace sai2b

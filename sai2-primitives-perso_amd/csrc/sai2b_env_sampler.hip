// sai2b_env_sampler.hip — env_randomize_kernel: the plant of the robots a mask selects redrawn in one launch (include/sai2b.h
// "environment sampler" has the law; sai2b_env_draw.h the draws, shared with the CPU). A stage of its own: every existing kernel
// keeps its instruction stream.
//
// One lane per robot, one wavefront per workgroup, every buffer [row][B]: a wavefront's 64 lanes touch 512 contiguous bytes per
// row. A wavefront without a selected robot leaves after its mask load (a uniform vote). The configuration is batch-uniform and
// travels as a kernel argument, so the ranges and the group bits sit in scalar registers and the group branches are uniform: a
// group that is not asked for costs no Philox call and no memory traffic. A lane reads and writes only its own column: no
// synchronisation, no LDS. Per group the traffic is the nominal rows in, the feature rows and the sample rows out; the arithmetic
// (at most 8 + 7 ceil(N / 4) Philox calls per robot for all groups) hides behind it. Loops over joints go in chunks of four, one
// Philox call each, fully unrolled (N is a compile-time constant), so nothing is indexed by a register.
// The two counts are reduced over the wavefront with shuffles and added by lane 0, one atomic each.
#include <hip/hip_runtime.h>

#include "../../include/sai2b.h"
#include "sai2b_launch.h"

namespace sai2b {
namespace {

__device__ __forceinline__ int env_wave_sum(int v) {
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
	return v;
}

// rows [first + 4 j .. first + 4 j + 3] (those below N) of a [.][B] buffer, column b; rows beyond N read as 1 and are not written
__device__ __forceinline__ void env_load4(const double* base, int first, int j, size_t sB, int b, double v[4]) {
#pragma unroll
	for (int i = 0; i < 4; i++) v[i] = 4 * j + i < N ? base[(size_t)(first + 4 * j + i) * sB + b] : 1.0;
}
__device__ __forceinline__ void env_store4(double* base, int first, int j, size_t sB, int b, const double v[4]) {
#pragma unroll
	for (int i = 0; i < 4; i++)
		if (4 * j + i < N) base[(size_t)(first + 4 * j + i) * sB + b] = v[i];
}

}  // namespace

__global__ __launch_bounds__(64) void env_randomize_kernel(const EnvParams P, const unsigned char* __restrict__ mask, const int B) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	const bool selected = b < B && mask[b < B ? b : B - 1] != 0;
	if (!__any(selected)) return;  // wave-uniform
	// (from here on every lane stays to the end: the counts are reduced over the whole wavefront)
	constexpr int CALLS = (N + 3) / 4;
	const size_t sB = (size_t)B;
	const unsigned robot = P.rng.first_robot + (unsigned)b, k0 = P.rng.key0, k1 = P.rng.key1;
	int clipped = 0;
	if (selected) {
		const unsigned c = (unsigned)P.counter[b];
		if (P.groups & SAI2B_ENV_PAYLOAD) {
			double s[4], nom[10], out[10];
			env_payload_sample(P.draw, c, robot, k0, k1, s);
#pragma unroll
			for (int k = 0; k < 4; k++) P.sample[(size_t)(P.sample_row[0] + k) * sB + b] = s[k];
#pragma unroll
			for (int k = 0; k < 10; k++) nom[k] = P.nom_plant_payload[(size_t)k * sB + b];
			env_payload_apply(s, nom, out);
#pragma unroll
			for (int k = 0; k < 10; k++) P.plant_payload[(size_t)k * sB + b] = out[k];
			if (P.both) {
#pragma unroll
				for (int k = 0; k < 10; k++) nom[k] = P.nom_payload[(size_t)k * sB + b];
				env_payload_apply(s, nom, out);
#pragma unroll
				for (int k = 0; k < 10; k++) P.payload[(size_t)k * sB + b] = out[k];
			}
		}
		if (P.groups & SAI2B_ENV_CONTACT) {
			double s[8], nom[9], out[9];
#pragma unroll
			for (int k = 0; k < 9; k++) nom[k] = P.nom_contact[(size_t)k * sB + b];
			env_contact(P.draw, c, robot, k0, k1, nom, out, s);
#pragma unroll
			for (int k = 0; k < 9; k++) P.contact[(size_t)k * sB + b] = out[k];
#pragma unroll
			for (int k = 0; k < 8; k++) P.sample[(size_t)(P.sample_row[1] + k) * sB + b] = s[k];
		}
		if (P.groups & SAI2B_ENV_JOINT_DYNAMICS) {
#pragma unroll
			for (int p = 0; p < ENV_JOINT_PARAMS; p++) {
#pragma unroll
				for (int j = 0; j < CALLS; j++) {
					double s[4], nom[4], out[4];
					env_load4(P.nom_joint, p * N, j, sB, b, nom);
					env_joint4(P.draw, p, j, c, robot, k0, k1, nom, out, s);
					env_store4(P.joint, p * N, j, sB, b, out);
					env_store4(P.sample, P.sample_row[2] + p * N, j, sB, b, s);
				}
			}
		}
		if (P.groups & SAI2B_ENV_HARDWARE) {
			const int row = P.sample_row[3];
			const double delay = env_delay(P.draw, c, robot, k0, k1);
			P.actuator[b] = delay;
			P.sample[(size_t)row * sB + b] = delay;
#pragma unroll
			for (int p = 0; p < ENV_HW_PARAMS; p++) {
#pragma unroll
				for (int j = 0; j < CALLS; j++) {
					double s[4], nom[4], out[4];
					env_load4(P.nom_actuator, 1 + p * N, j, sB, b, nom);
					const int clip = env_hardware4(P.draw, p, j, c, robot, k0, k1, nom, out, s);
					// (a lane beyond N of the last chunk holds 1 x s: never counted, never stored)
#pragma unroll
					for (int i = 0; i < 4; i++)
						if (4 * j + i < N && (clip >> i & 1)) clipped = 1;
					env_store4(P.actuator, 1 + p * N, j, sB, b, out);
					env_store4(P.sample, row + 1 + p * N, j, sB, b, s);
				}
			}
			double s[7], nom[12], out[12];
#pragma unroll
			for (int k = 0; k < 12; k++) nom[k] = P.nom_sensor[(size_t)k * sB + b];
			env_sensor(P.draw, c, robot, k0, k1, nom, out, s);
#pragma unroll
			for (int k = 0; k < 12; k++) P.sensor[(size_t)k * sB + b] = out[k];
#pragma unroll
			for (int k = 0; k < 7; k++) P.sample[(size_t)(row + 1 + ENV_HW_PARAMS * N + k) * sB + b] = s[k];
		}
		if (P.groups & SAI2B_ENV_PUSH) {
			double s[9], out[7];
			env_push(P.draw, c, robot, k0, k1, out, s);
#pragma unroll
			for (int k = 0; k < 7; k++) P.wrench[(size_t)k * sB + b] = out[k];
#pragma unroll
			for (int k = 0; k < 9; k++) P.sample[(size_t)(P.sample_row[4] + k) * sB + b] = s[k];
		}
		P.counter[b] = (int)(c + 1u);
	}
	const int n_drawn = env_wave_sum(selected ? 1 : 0);
	const int n_clipped = env_wave_sum(clipped);
	if (threadIdx.x == 0) {
		atomicAdd(P.counts + 0, n_drawn);
		if (n_clipped) atomicAdd(P.counts + 1, n_clipped);
	}
}

int launch_env_randomize(int B, const EnvParams& p, const unsigned char* mask, hipStream_t stream) {
	hipLaunchKernelGGL(env_randomize_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, p, mask, B);
	return launch_result();
}

}  // namespace sai2b

// sai2b_collision.hip — collision proximity and episodes ended from outside (include/sai2b.h "collision proximity"):
// collision_kernel evaluates the law of sai2b_collision_law.h for every robot in one launch; end_episodes_kernel closes the
// episodes of the robots a caller's byte mask names. Both are stages of their own, launched only by their own entry points:
// every existing kernel keeps its instruction stream, and a context that never calls them launches what it launched before.
//
// One lane per robot, one wavefront per workgroup, as sai2b_joint_sensor.hip. Every buffer is [row][B], so a wavefront's 64 lanes
// touch 512 contiguous bytes per row. A lane reads and writes only its own column: no LDS, no synchronisation. The geometry
// (which link a sphere sits on, which pairs are tested, which blocks are stored) is batch-uniform and arrives by value: the
// law tests it with scalar branches around unrolled code, so no array is indexed at run time.
//
// Counts: a ballot and one atomic add per wavefront and counter that has something to add (as observe_kernel; lane 0 always has
// a robot).
#include <hip/hip_runtime.h>

#include "sai2b_collision_law.h"
#include "sai2b_launch.h"

namespace sai2b {

__global__ __launch_bounds__(64) void collision_kernel(const ColParams P, const int B) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	const int flags = collision_law<N>(P.law, P.q + b, P.rows + b, (size_t)B, P.out ? P.out + b : nullptr);
	if (P.flags) P.flags[b] = (unsigned char)flags;
#pragma unroll
	for (int r = 0; r < COL_COUNTS; r++) {
		const unsigned long long hit = __ballot(r < COL_COUNTS - 1 ? ((flags >> r) & 1) != 0 : flags != 0);
		if (threadIdx.x == 0 && hit) atomicAdd(P.counts + r, __popcll(hit));
	}
}

// A robot with extra == 0 is neither read nor written. One that was already done keeps its bookkeeping and gains the bit.
__global__ __launch_bounds__(64) void end_episodes_kernel(const EndParams P, const int B) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	const size_t sB = (size_t)B;
	bool closed = false;
	if (P.extra[b] != 0) {
		const unsigned char d = P.done[b];
		if (d == 0) {
			closed = true;
			if (P.state) {
				P.state[REW_LAST_RETURN * sB + b] = P.state[REW_RET * sB + b];
				P.episode[b] = P.steps ? P.steps[b] : 0;
				P.state[REW_RET * sB + b] = 0.0;
				P.state[REW_DISC * sB + b] = 1.0;
				P.episode[sB + b] = 0;
			}
			if (P.steps) P.steps[b] = 0;
		}
		P.done[b] = (unsigned char)(d | P.bit);
	}
	const unsigned long long hit = __ballot(closed);
	if (threadIdx.x == 0 && hit) atomicAdd(P.count, __popcll(hit));
}

int launch_collision(int B, const ColParams& p, hipStream_t stream) {
	hipLaunchKernelGGL(collision_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, p, B);
	return launch_result();
}

int launch_end_episodes(int B, const EndParams& p, hipStream_t stream) {
	hipLaunchKernelGGL(end_episodes_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, p, B);
	return launch_result();
}

}  // namespace sai2b

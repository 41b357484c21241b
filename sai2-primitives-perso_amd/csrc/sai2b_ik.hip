// sai2b_ik.hip — inverse kinematics for every robot (include/sai2b.h "inverse kinematics"): ik_kernel runs the law of
// sai2b_ik_law.h for the robots a byte mask selects, in one launch. A stage of its own, launched only by sai2b_solve_ik: every
// existing kernel keeps its instruction stream, and a context that never calls it launches what it launched before.
//
// One lane per robot, one wavefront per workgroup, FP64 in registers, no LDS. Every buffer is [row][B], so a wavefront's 64 lanes
// touch 512 contiguous bytes per row; a lane reads and writes only its own column. The configuration (the chain, the task's link
// and control frame, the clamped limits, the schedule) is batch-uniform and arrives by value: the law tests it with scalar
// branches around unrolled code, so no array is indexed at run time.
//
// A wavefront with no selected robot leaves after its mask load. The others run the law's loop until no lane has work left: the
// wavefront pays for its slowest robot (measured: DESIGN 8s). A lane beyond B, an unselected one and one whose inputs are not
// finite pass through the loop with their execution bit off and touch no memory.
//
// Counts: the four per-lane bits are packed into one word of 8-bit fields (a field holds at most 64), summed over the wavefront
// by a butterfly of shuffles, and lane 0 adds every non-zero field with one atomic.
#include <hip/hip_runtime.h>

#include "sai2b_ik_law.h"
#include "sai2b_launch.h"

namespace sai2b {

__global__ __launch_bounds__(64) void ik_kernel(const IkParams P, const int B) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	const bool live = b < B && (P.mask ? P.mask[b] != 0 : true);
	if (!__any(live)) return;  // wave-uniform
	const size_t col = live ? (size_t)b : 0;
	const int flags = ik_law<N>(P.law, live, P.goal + col, P.rest ? P.rest + col : nullptr, P.seed + col, (size_t)B, (unsigned)b, P.q_out + col,
								P.status + col);
	if (live) P.flags[b] = (unsigned char)flags;
	int packed = live ? (1 | ((flags & IK_FLAG_CONVERGED) ? 1 << 8 : 0) | ((flags & IK_FLAG_EXHAUSTED) ? 1 << 16 : 0) |
						 ((flags & IK_FLAG_NONFINITE) ? 1 << 24 : 0))
					  : 0;
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) packed += __shfl_xor(packed, m, 64);
	if (threadIdx.x == 0) {
#pragma unroll
		for (int r = 0; r < IK_COUNTS; r++) {
			const int n = (packed >> (8 * r)) & 255;
			if (n) atomicAdd(P.counts + r, n);
		}
	}
}

int launch_ik(int B, const IkParams& p, hipStream_t stream) {
	hipLaunchKernelGGL(ik_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, p, B);
	return launch_result();
}

}  // namespace sai2b

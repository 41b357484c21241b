// sai2b_observe.hip — observations and episode-end flags for every robot in one launch (include/sai2b.h "observations
// and episode-end flags"): the producer of the done mask that sai2b_reset_robots consumes, so that the loop
// tick -> sim_step -> observe -> reset never leaves the device.
//
// One lane per robot, one wavefront per workgroup, as everywhere in this library. One fk() per robot serves every observed
// task; per task only what a selected block or an enabled criterion needs is computed (the selection is batch-uniform, so
// these are uniform branches). The quantities are the ones the host getters report (mft_status_kernel in sai2b_sim.hip),
// through the same device functions. Stores are SoA [row][B]. The kernel's parameters (ObsParams, sai2b_launch.h) are a
// kernel argument of their own: DevParams and every other kernel are as they were.
//
// The kernel's text (sai2b_observe_body.inc) serves two kernels through a compile-time switch: observe_kernel (OBSERVE_REWARD 0)
// is what it always was, observe_reward_kernel (OBSERVE_REWARD 1; include/sai2b.h "rewards and episode returns") evaluates in
// the same launch the reward terms from the intermediates the observation computes anyway, sums them and keeps the per-robot
// episode accumulators.
#include <hip/hip_runtime.h>

#include "sai2b_device.hpp"
#include "sai2b_launch.h"

namespace sai2b {

// rows of the per-task blocks, in flag order
constexpr int OBS_POSE_ROWS = 12, OBS_TWIST_ROWS = 6, OBS_ERROR_ROWS = 8, OBS_SENSED_ROWS = 6;

// task terms by the observation intermediate they read
constexpr int REW_NEED_ERROR = SAI2B_REW_POS | SAI2B_REW_POS_SQ | SAI2B_REW_POS_TANH | SAI2B_REW_ORI | SAI2B_REW_ORI_SQ | SAI2B_REW_ORI_TANH;
constexpr int REW_NEED_TWIST = SAI2B_REW_LIN_VEL_SQ | SAI2B_REW_ANG_VEL_SQ;
constexpr int REW_NEED_SENSED = SAI2B_REW_FORCE_ERR_SQ | SAI2B_REW_FORCE_EXCESS;
constexpr int REW_BIT_POS = 0, REW_BIT_POS_SQ = 1, REW_BIT_POS_TANH = 2, REW_BIT_ORI = 3, REW_BIT_ORI_SQ = 4, REW_BIT_ORI_TANH = 5,
			  REW_BIT_LIN_VEL_SQ = 6, REW_BIT_ANG_VEL_SQ = 7, REW_BIT_FORCE_ERR_SQ = 8, REW_BIT_FORCE_EXCESS = 9;

// observe_reward_kernel alone: a robot's task terms, [task term row][lane], between the task loop that computes them and the sum
// that takes them in layout order behind the DONE term (which needs the byte the loop's criteria decide). Every lane reads what
// it wrote itself: no barrier. Sized by the launch: task term rows * 64 doubles.
extern __shared__ real rew_task_terms[];

// r + w * v as a multiply and an add of their own: hipcc contracts across statements unless told otherwise, and the reward and
// the return are defined (and tested, bit for bit) as the unfused forms
DI real rew_mul_add(real r, real w, real v) {
#pragma clang fp contract(off)
	const real p = w * v;
	return r + p;
}

// the kernel's text, once for each of the two kernels
#define OBSERVE_REWARD 0
#define REW_OR(x)
#include "sai2b_observe_body.inc"
#undef OBSERVE_REWARD
#undef REW_OR
#define OBSERVE_REWARD 1
#define REW_OR(x) || (x)
#include "sai2b_observe_body.inc"
#undef OBSERVE_REWARD
#undef REW_OR

// sai2b_reset_robots with a reward configured: the selected robots start a new return
__global__ __launch_bounds__(64) void reward_reset_kernel(int B, const unsigned char* __restrict__ mask, real* __restrict__ state,
														   int* __restrict__ episode) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	if (!((const __attribute__((address_space(1))) unsigned char*)mask)[b]) return;
	st(state, REW_RET, B, b, 0.0);
	st(state, REW_DISC, B, b, 1.0);
	sti(episode, 1, B, b, 0);
}

int launch_observe(const DevParams* d_params, int B, const ObsParams& obs, double* out, unsigned char* done, int* steps, int* counts,
				   hipStream_t stream) {
	hipLaunchKernelGGL(observe_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_params, obs, out, done, steps, counts);
	return launch_result();
}

int launch_observe_reward(const DevParams* d_params, int B, const ObsParams& obs, const RewParams& rew, double* out, unsigned char* done,
						  int* steps, int* counts, hipStream_t stream) {
	const size_t lds = (size_t)rew.task_rows * 64 * sizeof(double);
	hipLaunchKernelGGL(observe_reward_kernel, dim3((B + 63) / 64), dim3(64), lds, stream, d_params, obs, rew, out, done, steps, counts);
	return launch_result();
}

int launch_reward_reset(int B, const unsigned char* mask, double* state, int* episode, hipStream_t stream) {
	hipLaunchKernelGGL(reward_reset_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, B, mask, state, episode);
	return launch_result();
}

}  // namespace sai2b

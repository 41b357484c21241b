// sai2b_joint_sensor.hip — the controller's view of the joint state (include/sai2b.h "joint sensors"): joint_sense_kernel turns
// the plant's q, dq into the measured pair the tick, the observation and the action read. It is a stage of its own behind the
// simulation kernel (and behind sense_kernel where that runs), not another form of an existing kernel: every existing kernel
// keeps its instruction stream. The law of one reading is sai2b_joint_sensor_law.h, shared with a CPU program.
//
// SEED = true: reading 0 of the robots a [B] byte mask selects (NULL: all), optionally of their next episode; the clock is left at
// 1. SEED = false: reading c of every robot, the clock is left at c + 1, and the measured q the last tick read is saved into
// q_pose first when the host asks (the tasks' cached pose, while the measured buffer still held it).
//
// One lane per robot, one wavefront per workgroup, as sai2b_hardware.hip. Every buffer is [row][B], so a wavefront's 64 lanes
// touch 512 contiguous bytes per row; the history is [slot][2 dof][B] and the lanes of a wavefront may read different slots (the
// delay is per robot), each still its own column. A lane reads and writes only its own column, so the kernel needs no
// synchronisation. Loops over joints are unrolled (N is a compile-time constant). No LDS.
//
// Noise: counter (reading, episode, 256 * 10 + call, first_robot + b). A wavefront whose deviation rows are all zero does not
// draw; a lane whose own deviation is zero takes its value as it is, so the result of a robot does not depend on whether its
// neighbours made the wavefront draw. The clock is an int, as the hardware's: see include/sai2b.h for its limit.
#include <hip/hip_runtime.h>

#include "sai2b_joint_sensor_law.h"
#include "sai2b_launch.h"

namespace sai2b {

template <bool SEED>
__global__ __launch_bounds__(64) void joint_sense_kernel(const JointSenseParams P, const int B) {
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	if (SEED && P.mask && P.mask[b] == 0) return;
	const size_t sB = (size_t)B;
	int m, e = P.clock[sB + b];
	if (SEED) {
		m = 0;
		if (P.next_episode) {
			e += 1;
			P.clock[sB + b] = e;
		}
		P.clock[b] = 1;
	} else {
		m = P.clock[b];
		P.clock[b] = m + 1;
	}
	const double* R = P.rows + b;
	const bool draw = __any(joint_sensor_noisy<N>(R, sB));
	joint_sensor_reading<N>(R, sB, P.q + b, P.dq + b, P.dt, m, e, P.velocity_mode, P.depth, draw, P.rng.key0, P.rng.key1,
							P.rng.first_robot + (unsigned)b, P.prev + b, P.filter + b, P.history + b, P.q_meas + b, P.dq_meas + b,
							(!SEED && P.q_pose) ? P.q_pose + b : nullptr);
}

int launch_joint_sense(int B, const JointSenseParams& p, bool seed, hipStream_t stream) {
	if (seed)
		hipLaunchKernelGGL(joint_sense_kernel<true>, dim3((B + 63) / 64), dim3(64), 0, stream, p, B);
	else
		hipLaunchKernelGGL(joint_sense_kernel<false>, dim3((B + 63) / 64), dim3(64), 0, stream, p, B);
	return launch_result();
}

}  // namespace sai2b

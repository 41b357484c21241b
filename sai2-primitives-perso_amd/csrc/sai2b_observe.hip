// sai2b_observe.hip — observations and episode-end flags for every robot in one launch (include/sai2b.h "observations
// and episode-end flags"): the producer of the done mask that sai2b_reset_robots consumes, so that the loop
// tick -> sim_step -> observe -> reset never leaves the device.
//
// One lane per robot, one wavefront per workgroup, as everywhere in this library. One fk() per robot serves every observed
// task; per task only what a selected block or an enabled criterion needs is computed (the selection is batch-uniform, so
// these are uniform branches). The quantities are the ones the host getters report (mft_status_kernel in sai2b_sim.hip),
// through the same device functions. Stores are SoA [row][B]. The kernel's parameters (ObsParams, sai2b_launch.h) are a
// kernel argument of their own: DevParams and every other kernel are as they were.
#include <hip/hip_runtime.h>

#include "sai2b_device.hpp"
#include "sai2b_launch.h"

namespace sai2b {

// rows of the per-task blocks, in flag order
constexpr int OBS_POSE_ROWS = 12, OBS_TWIST_ROWS = 6, OBS_ERROR_ROWS = 8, OBS_SENSED_ROWS = 6;

__global__ __launch_bounds__(64) void observe_kernel(const DevParams* __restrict__ Pp, const ObsParams O, real* __restrict__ out,
													  unsigned char* __restrict__ done, int* __restrict__ steps, int* __restrict__ counts) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	real q[N], dq[N];
	bool finite = true;
	UNROLL for (int i = 0; i < N; i++) {
		q[i] = ld(P.q, i, B, b);
		dq[i] = ld(P.dq, i, B, b);
		finite = finite && isfinite(q[i]) && isfinite(dq[i]);
	}
	// ---- global blocks and the criteria that need no kinematics
	real margin = q[0] - P.model.q_lower[0];
	bool speeding = false;
	UNROLL for (int i = 0; i < N; i++) {
		margin = fmin(margin, fmin(q[i] - P.model.q_lower[i], P.model.q_upper[i] - q[i]));
		speeding = speeding || fabs(dq[i]) > O.max_speed[i];
	}
	const int step = ldi(steps, 0, B, b) + 1;
	if (out) {
		if (O.blocks & SAI2B_OBS_Q) {
			UNROLL for (int i = 0; i < N; i++) st(out, O.row_global[0] + i, B, b, q[i]);
		}
		if (O.blocks & SAI2B_OBS_DQ) {
			UNROLL for (int i = 0; i < N; i++) st(out, O.row_global[1] + i, B, b, dq[i]);
		}
		if (O.blocks & SAI2B_OBS_TAU) {
			UNROLL for (int i = 0; i < N; i++) st(out, O.row_global[2] + i, B, b, ld(P.tau, i, B, b));
		}
		if (O.blocks & SAI2B_OBS_LIMIT_MARGIN) st(out, O.row_global[3], B, b, margin);
		if (O.blocks & SAI2B_OBS_EPISODE_STEP) st(out, O.row_global[4], B, b, (real)step);
		if (O.blocks & SAI2B_OBS_CONTACT) {
			const bool have = P.contact_status != nullptr;	// batch-uniform; the rows are zeroed when a contact is cleared
#pragma unroll 1
			for (int k = 0; k < CONTACT_STATUS_ROWS; k++) st(out, O.row_global[5] + k, B, b, have ? ld(P.contact_status, k, B, b) : 0.0);
		}
	}
	// ---- tasks: observed ones, and those a criterion reads
	const int success_mask = (O.criteria & SAI2B_DONE_SUCCESS) ? O.success_mask : 0;
	const int force_mask = (O.criteria & SAI2B_DONE_FORCE) ? O.force_mask : 0;
	const int stored_mask = out ? O.task_mask : 0;
	const int visit_mask = (stored_mask && O.task_blocks ? stored_mask : 0) | success_mask | force_mask;
	bool success = true, overforce = false;
	if (visit_mask) {
		Frames F;
		fk(P.model, q, F);
#pragma unroll 1
		for (int k = 0; k < SAI2B_MAX_TASKS; k++) {
			if (!((visit_mask >> k) & 1)) continue;
			const DevTask& t = P.task[k];
			const int tb = ((stored_mask >> k) & 1) ? O.task_blocks : 0;
			int row = O.row_task[k];
			real x[3], R[9];
			frame_pose(t, F, x, R);
			if (tb & SAI2B_OBS_POSE) {
				UNROLL for (int a = 0; a < 3; a++) st(out, row + a, B, b, x[a]);
				UNROLL for (int a = 0; a < 9; a++) st(out, row + 3 + a, B, b, R[a]);
				row += OBS_POSE_ROWS;
			}
			if (tb & SAI2B_OBS_TWIST) {
				real J[6 * N], v[6];
				jacobian(P.model, t, F, x, J);
				mv<6, N>(J, dq, v);
				UNROLL for (int a = 0; a < 6; a++) st(out, row + a, B, b, v[a]);
				row += OBS_TWIST_ROWS;
			}
			const bool for_success = (success_mask >> k) & 1;
			if ((tb & SAI2B_OBS_ERROR) || for_success) {
				real sf[9], sp[9], sm[9], so[9], gpos[3], grot[9], e[3], oe[3], se[3], soe[3];
				sigma_pair(t, 0, t.fdim, t.faxis, R, sf, sp);
				sigma_pair(t, 1, t.mdim, t.maxis, R, sm, so);
				UNROLL for (int a = 0; a < 3; a++) gpos[a] = ld(t.goals, MFT_GOAL_POS + a, B, b);
				UNROLL for (int a = 0; a < 9; a++) grot[a] = ld(t.goals, MFT_GOAL_ROT + a, B, b);
				UNROLL for (int a = 0; a < 3; a++) e[a] = gpos[a] - x[a];
				orientation_error(grot, R, oe);
				mv3(sp, e, se);
				mv3(so, oe, soe);
				// the rows clamp as mft_status_kernel does; fmax drops a NaN, so the criterion looks at the unclamped forms
				const real p2 = e[0] * se[0] + e[1] * se[1] + e[2] * se[2], o2 = oe[0] * soe[0] + oe[1] * soe[1] + oe[2] * soe[2];
				const real pn = sqrt(fmax(p2, 0.0)), on = sqrt(fmax(o2, 0.0));
				if (tb & SAI2B_OBS_ERROR) {
					UNROLL for (int a = 0; a < 3; a++) {
						st(out, row + a, B, b, se[a]);
						st(out, row + 3 + a, B, b, soe[a]);
					}
					st(out, row + 6, B, b, pn);
					st(out, row + 7, B, b, on);
					row += OBS_ERROR_ROWS;
				}
				// goalPositionReached && goalOrientationReached, strict (MotionForceTask.cpp:548-579); a NaN error (a goal row
				// that is not finite under a finite state): not reached
				if (for_success) success = success && p2 == p2 && o2 == o2 && (pn < O.pos_tol) && (on < O.ori_tol);
			}
			const bool for_force = (force_mask >> k) & 1;
			if ((tb & SAI2B_OBS_SENSED) || for_force) {
				real sfc[3], smc[3], fs_w[3], ms_w[3];
				UNROLL for (int a = 0; a < 3; a++) {
					sfc[a] = ld(t.sensed, a, B, b);
					smc[a] = ld(t.sensed, 3 + a, B, b);
				}
				sensed_wrench_world(t, R, sfc, smc, fs_w, ms_w);
				if (tb & SAI2B_OBS_SENSED) {
					UNROLL for (int a = 0; a < 3; a++) {
						st(out, row + a, B, b, fs_w[a]);
						st(out, row + 3 + a, B, b, ms_w[a]);
					}
					row += OBS_SENSED_ROWS;
				}
				if (for_force) overforce = overforce || sqrt(fs_w[0] * fs_w[0] + fs_w[1] * fs_w[1] + fs_w[2] * fs_w[2]) > O.max_force;
			}
		}
	}
	// ---- the done byte. The criteria that read the state are not evaluated on a state that is not finite.
	int bits = 0;
	if ((O.criteria & SAI2B_DONE_SUCCESS) && finite && success) bits |= SAI2B_DONE_SUCCESS;
	if ((O.criteria & SAI2B_DONE_JOINT_LIMIT) && finite && margin < O.limit_margin) bits |= SAI2B_DONE_JOINT_LIMIT;
	if ((O.criteria & SAI2B_DONE_SPEED) && finite && speeding) bits |= SAI2B_DONE_SPEED;
	if ((O.criteria & SAI2B_DONE_NONFINITE) && !finite) bits |= SAI2B_DONE_NONFINITE;
	if ((O.criteria & SAI2B_DONE_FORCE) && finite && overforce) bits |= SAI2B_DONE_FORCE;
	if ((O.criteria & SAI2B_DONE_TIMEOUT) && step >= O.max_steps) bits |= SAI2B_DONE_TIMEOUT;
	if (done) ((__attribute__((address_space(1))) unsigned char*)done)[b] = (unsigned char)bits;
	sti(steps, 0, B, b, bits ? 0 : step);
	// counts per reason and of robots that are done: one atomic per wavefront and counter that has something to add
	// (as contact_count in sai2b_sim.hip; lane 0 always has a robot)
	if (O.criteria) {
		UNROLL for (int r = 0; r < OBS_COUNTS; r++) {
			const unsigned long long hit = __ballot(r < SAI2B_DONE_REASONS ? ((bits >> r) & 1) != 0 : bits != 0);
			if (threadIdx.x == 0 && hit) atomicAdd(counts + r, __popcll(hit));
		}
	}
}

int launch_observe(const DevParams* d_params, int B, const ObsParams& obs, double* out, unsigned char* done, int* steps, int* counts,
				   hipStream_t stream) {
	hipLaunchKernelGGL(observe_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_params, obs, out, done, steps, counts);
	return launch_result();
}

}  // namespace sai2b

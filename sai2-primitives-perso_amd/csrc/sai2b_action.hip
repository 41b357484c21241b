// sai2b_action.hip — a policy's action rows to the goal rows of the chosen tasks, for every robot in one launch
// (include/sai2b.h "actions"): the consumer side of the loop tick -> sim_step -> observe -> policy -> apply_action -> reset.
//
// One lane per robot, one wavefront per workgroup, as everywhere in this library. The configuration is batch-uniform, so
// every branch on it is uniform; the only per-lane branches are the mask and the rejection of a robot whose action (or,
// where the configuration reads it, state) is not finite. The action is read twice: once to decide whether the robot is
// accepted at all (none of its rows may be written otherwise), once to map it; the second read hits the cache. One fk() per
// robot serves every task, and only when some task needs the current pose. Loads and stores are SoA [row][B]. The kernel's
// parameters (ActParams, sai2b_launch.h) are a kernel argument of their own: DevParams and every other kernel are as they
// were.
#include <hip/hip_runtime.h>

#include "sai2b_device.hpp"
#include "sai2b_launch.h"

namespace sai2b {

// below this th^2 the exponential's coefficients come from their series (sai2b.h "actions")
constexpr real ACT_EXP_SERIES_TH2 = 1e-8;

// v limited to [-1, 1] when clip is set; a NaN passes through (the robot is rejected before this is used)
DI real act_clip(real v, int clip) { return clip ? (v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v)) : v; }
// v into [lo, hi]; *hit when it moved. A NaN v compares false twice and stays.
DI real act_clamp(real v, real lo, real hi, bool* hit) {
	if (v < lo) {
		*hit = true;
		return lo;
	}
	if (v > hi) {
		*hit = true;
		return hi;
	}
	return v;
}

__global__ __launch_bounds__(64) void action_kernel(const DevParams* __restrict__ Pp, const ActParams A, const real* __restrict__ action,
													 const unsigned char* __restrict__ mask, int* __restrict__ counts) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	const bool selected = !mask || ((const __attribute__((address_space(1))) unsigned char*)mask)[b] != 0;
	bool rejected = false, clipped = false, limited = false;
	if (selected) {
		// ---- accepted or not: every action component finite, and the state where it is read
		bool ok = true;
#pragma unroll 1
		for (int r = 0; r < A.rows; r++) {
			const real v = ld(action, r, B, b);
			ok = ok && isfinite(v);
			clipped = clipped || fabs(v) > 1.0;
		}
		real q[N];
		if (A.need_state) {
			UNROLL for (int i = 0; i < N; i++) {
				q[i] = ld(P.q, i, B, b);
				ok = ok && isfinite(q[i]);
			}
		}
		rejected = !ok;
		clipped = clipped && A.clip && ok;
		if (ok) {
			Frames F;
			if (A.need_pose) fk(P.model, q, F);
#pragma unroll 1
			for (int k = 0; k < SAI2B_MAX_TASKS; k++) {
				const ActTask& a = A.task[k];
				if (a.mode == SAI2B_ACT_NONE) continue;
				const DevTask& t = P.task[k];
				int row = a.row;
				if (t.type == SAI2B_JOINT_TASK) {
					UNROLL for (int i = 0; i < N; i++) {
						if (i < t.k0) {
							real base = 0.0;
							if (a.mode == SAI2B_ACT_DELTA_GOAL) base = ld(t.goals, i, B, b);
							if (a.mode == SAI2B_ACT_DELTA_CURRENT) {
								if (t.full_selection) {
									base = q[i];
								} else {
									UNROLL for (int j = 0; j < N; j++) base = fma(t.S[i * N + j], q[j], base);
								}
							}
							const real g = fma(a.jt_scale[i], act_clip(ld(action, row + i, B, b), A.clip), base);
							st(t.goals, i, B, b, act_clamp(g, a.jt_lower[i], a.jt_upper[i], &limited));
						}
					}
					continue;
				}
				const bool lead = a.max_lead < INFINITY;
				const bool pose = a.mode == SAI2B_ACT_DELTA_CURRENT || ((a.blocks & SAI2B_ACT_POSITION) && lead);
				real x[3], R[9];
				if (pose) frame_pose(t, F, x, R);
				if (a.blocks & SAI2B_ACT_POSITION) {
					real p[3];
					UNROLL for (int c = 0; c < 3; c++) {
						real base = 0.0;
						if (a.mode == SAI2B_ACT_DELTA_GOAL) base = ld(t.goals, MFT_GOAL_POS + c, B, b);
						if (a.mode == SAI2B_ACT_DELTA_CURRENT) base = x[c];
						p[c] = fma(a.pos_scale[c], act_clip(ld(action, row + c, B, b), A.clip), base);
						p[c] = act_clamp(p[c], a.pos_lower[c], a.pos_upper[c], &limited);
					}
					if (lead) {
						const real e[3] = {p[0] - x[0], p[1] - x[1], p[2] - x[2]};
						const real n = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
						if (n > a.max_lead) {
							const real s = a.max_lead / n;
							UNROLL for (int c = 0; c < 3; c++) p[c] = fma(e[c], s, x[c]);
							limited = true;
						}
					}
					UNROLL for (int c = 0; c < 3; c++) st(t.goals, MFT_GOAL_POS + c, B, b, p[c]);
					row += 3;
				}
				if (a.blocks & SAI2B_ACT_ORIENTATION) {
					real w[3], Rb[9];
					UNROLL for (int c = 0; c < 3; c++) w[c] = a.ori_scale * act_clip(ld(action, row + c, B, b), A.clip);
					if (a.mode == SAI2B_ACT_DELTA_GOAL) {
						UNROLL for (int c = 0; c < 9; c++) Rb[c] = ld(t.goals, MFT_GOAL_ROT + c, B, b);
					} else if (a.mode == SAI2B_ACT_DELTA_CURRENT) {
						UNROLL for (int c = 0; c < 9; c++) Rb[c] = R[c];
					} else {
						UNROLL for (int c = 0; c < 9; c++) Rb[c] = (c % 4 == 0) ? 1.0 : 0.0;
					}
					const real th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
					real ca, cb;
					if (th2 < ACT_EXP_SERIES_TH2) {
						ca = 1.0 - th2 / 6.0;
						cb = 0.5 - th2 / 24.0;
					} else {
						const real th = sqrt(th2), sh = sin(0.5 * th);
						ca = sin(th) / th;
						cb = 2.0 * sh * sh / th2;
					}
					// D = A [w]x + B [w]x^2, with [w]x^2 = w w^T - th2 I; R_new = R_base + D R_base
					real D[9], DR[9];
					D[0] = -cb * (w[1] * w[1] + w[2] * w[2]);
					D[4] = -cb * (w[0] * w[0] + w[2] * w[2]);
					D[8] = -cb * (w[0] * w[0] + w[1] * w[1]);
					D[1] = cb * w[0] * w[1] - ca * w[2];
					D[3] = cb * w[0] * w[1] + ca * w[2];
					D[2] = cb * w[0] * w[2] + ca * w[1];
					D[6] = cb * w[0] * w[2] - ca * w[1];
					D[5] = cb * w[1] * w[2] - ca * w[0];
					D[7] = cb * w[1] * w[2] + ca * w[0];
					mm<3, 3, 3>(D, Rb, DR);
					UNROLL for (int c = 0; c < 9; c++) st(t.goals, MFT_GOAL_ROT + c, B, b, Rb[c] + DR[c]);
					row += 3;
				}
				if (a.blocks & SAI2B_ACT_FORCE) {
					UNROLL for (int c = 0; c < 3; c++)
						st(t.goals, MFT_GOAL_FORCE + c, B, b, a.force_scale * act_clip(ld(action, row + c, B, b), A.clip));
					row += 3;
				}
				if (a.blocks & SAI2B_ACT_MOMENT) {
					UNROLL for (int c = 0; c < 3; c++)
						st(t.goals, MFT_GOAL_MOMENT + c, B, b, a.moment_scale * act_clip(ld(action, row + c, B, b), A.clip));
				}
			}
		}
	}
	// counts of robots rejected, clipped and limited: one atomic per wavefront and counter that has something to add (as
	// observe_kernel; a rejected robot has no other flag)
	const bool flag[ACT_COUNTS] = {rejected, clipped, limited && !rejected};
	UNROLL for (int r = 0; r < ACT_COUNTS; r++) {
		const unsigned long long hit = __ballot(flag[r]);
		if (threadIdx.x == 0 && hit) atomicAdd(counts + r, __popcll(hit));
	}
}

int launch_action(const DevParams* d_params, int B, const ActParams& act, const double* action, const unsigned char* mask, int* counts,
				  hipStream_t stream) {
	hipLaunchKernelGGL(action_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_params, act, action, mask, counts);
	return launch_result();
}

}  // namespace sai2b

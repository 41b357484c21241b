// sai2b_kernels.hip — gfx950 kernels of the batched operational-space controller.
//
// tick_kernel: one launch = RobotController::updateControllerTaskModels() +
// computeControlTorques() (reference src/RobotController.cpp:53-74) for B robots, preceded by the
// model update the reference gets from Sai2Model::updateModel(). One lane per robot, 64-thread
// workgroups (one wavefront each) so that B/64 workgroups spread over all 1024 SIMDs.
#include <hip/hip_runtime.h>

#include "sai2b_device.hpp"
#include "sai2b_fast_body.hpp"
#include "sai2b_launch.h"

namespace sai2b {

// Generic tick: Jacobi-SVD based, any hierarchy (the reference's control flow, projector form).
// fb_count != NULL: the fallback pass behind tick_fast_kernel — lane i of the grid takes robot
// fb_list[i] for i < *fb_count (the robots the SVD-free kernel declined, compacted), the rest exits.
// RANGE: the pass ahead of the generator kernels that only decides which robots' gated JointTasks have a
// range this tick (DevTask::otg_gated): nothing after the last such task is needed. A separate
// instantiation, so that the tick proper compiles as it did without it.
template <bool DEBUG, bool RANGE = false>
__global__ __launch_bounds__(64) void tick_kernel(const DevParams* __restrict__ Pp, int commit_sh, int with_comp,
													 int do_torque, const int* __restrict__ fb_count,
													 const int* __restrict__ fb_list) {
	const DevParams& P = *Pp;
	const int B = P.B;
	int b = blockIdx.x * 64 + threadIdx.x;
	if (fb_count) {
		if (b >= *(const gint*)fb_count) return;
		b = ((const gint*)fb_list)[b];
	}
	if (b >= B) return;
	RobotCtx rc;
	UNROLL for (int i = 0; i < N; i++) {
		rc.q[i] = ld(P.q, i, B, b);
		rc.dq[i] = ld(P.dq, i, B, b);
	}
	real g[N];
	{
		// never the hot route: one kernel for contexts with and without payloads, a wave-uniform branch around the payload's
		// work (without rows the calls are the ones this kernel always made)
		Payload pl;
		payload_load(P.payload, P.payload_link, B, b, pl);
		// Sai2Model::updateModel(): kinematics, M (CRBA), M^-1 (examples/05-using_robot_controller.cpp:143-145)
		Frames F;
		fk(P.model, rc.q, F);
		real M[N * N];
		if (P.payload)
			mass_matrix(P.model, F, M, pl);
		else
			mass_matrix(P.model, F, M);
		spd_inverse<N>(M, rc.Minv);
		if (DEBUG && P.dbg_M) {
			UNROLL for (int i = 0; i < N * N; i++) st(P.dbg_M, i, B, b, M[i]);
		}
		// bounded inertia estimate (SingularityHandler.cpp:176-182, JointTask.cpp:254-260), shared by
		// every task with the same threshold (the reference recomputes it per task: SURVEY App. B-8)
		bool any_bie = false;
		real thr = 0;
		for (int t = 0; t < P.n_tasks; t++)
			if (P.task[t].decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES) {
				any_bie = true;
				thr = P.task[t].bie_threshold;
			}
		if (any_bie) {
			UNROLL for (int i = 0; i < N; i++) M[i * N + i] = fmax(M[i * N + i], thr);
			spd_inverse<N>(M, rc.MinvB);
		} else {
			UNROLL for (int i = 0; i < N * N; i++) rc.MinvB[i] = rc.Minv[i];
		}
		if (P.gravity_comp && P.payload)
			gravity_vector(P.model, F, g, pl);
		else if (P.gravity_comp)
			gravity_vector(P.model, F, g);
		else {
			UNROLL for (int i = 0; i < N; i++) g[i] = 0;
		}
	}
	real Nprec[N * N], tau[N];
	UNROLL for (int i = 0; i < N * N; i++) Nprec[i] = (i % (N + 1) == 0) ? 1.0 : 0.0;
	UNROLL for (int i = 0; i < N; i++) tau[i] = 0;
	Chain chain;
	chain.ok = !DEBUG;
	chain.wrows = 0;
	UNROLL for (int i = 0; i < N * N; i++) chain.W[i] = 0;
	int n_run = P.n_tasks;
	if constexpr (RANGE) {
		n_run = 0;
		for (int t = 0; t < P.n_tasks; t++)
			if (P.task[t].otg_gated) n_run = t + 1;
	}
#pragma unroll 1
	for (int t = 0; t < n_run; t++) {
		const DevTask& tk = P.task[t];
		const bool first = (t == 0), last = (t == P.n_tasks - 1);
		if (tk.type == SAI2B_MOTION_FORCE_TASK)
			mft_task<DEBUG>(P, tk, rc, B, b, first, last, commit_sh != 0, do_torque != 0, Nprec, tau, chain);
		else if (RANGE && t == n_run - 1)
			jt_task<DEBUG, true>(P, tk, rc, B, b, first, last, with_comp != 0, do_torque != 0, Nprec, tau, chain);
		else
			jt_task<DEBUG>(P, tk, rc, B, b, first, last, with_comp != 0, do_torque != 0, Nprec, tau, chain);
	}
	if (do_torque) {
		UNROLL for (int i = 0; i < N; i++) st(P.tau, i, B, b, tau[i] + g[i]);  // RobotController.cpp:70-72
	}
}

#if SAI2B_N == 7  // the SVD-free kernels are for 7-joint robots: their per-lane body is sai2b_fast_body.hpp
template <int FAST, bool BAKED>
__global__ __launch_bounds__(64) void tick_fast_kernel(const DevParams* __restrict__ Pp, int with_comp,
														  int* __restrict__ fb_counts, int* __restrict__ fb_list,
														  int parity) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b0 = blockIdx.x * 64, b = b0 + threadIdx.x;
	// (and the in-lane branch's count of the next launch: tick_cert_kernel<6, S6> may follow this kernel and adds to it)
	// [4 + ..]: the largest number of declined robots in one wavefront (worklist_append through fast_declined)
	if (blockIdx.x == 0 && threadIdx.x == 0)
		((gint*)fb_counts)[1 - parity] = 0, ((gint*)fb_counts)[2 + (1 - parity)] = 0, ((gint*)fb_counts)[4 + (1 - parity)] = 0;
	if constexpr (FAST == 1) {
		if (b < B) tick_fast1_loads<BAKED, NoPayload>(P, with_comp, fb_counts, fb_list, parity, b);
		return;
	}
	__shared__ real img[StageLayout<FAST>::DOUBLES];
	tick_fast_body<FAST, BAKED, NoPayload>(Pp, with_comp, fb_counts, fb_list, parity, img);
}
// the same tick with each robot's payload added to its M and g (selected by the host: sai2b_set_link_payload)
template <int FAST, bool BAKED>
__global__ __launch_bounds__(64) void tick_fast_payload_kernel(const DevParams* __restrict__ Pp, int with_comp,
																  int* __restrict__ fb_counts, int* __restrict__ fb_list,
																  int parity) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b0 = blockIdx.x * 64, b = b0 + threadIdx.x;
	// (and the in-lane branch's count of the next launch: tick_cert_kernel<6, S6> may follow this kernel and adds to it)
	// [4 + ..]: the largest number of declined robots in one wavefront (worklist_append through fast_declined)
	if (blockIdx.x == 0 && threadIdx.x == 0)
		((gint*)fb_counts)[1 - parity] = 0, ((gint*)fb_counts)[2 + (1 - parity)] = 0, ((gint*)fb_counts)[4 + (1 - parity)] = 0;
	if constexpr (FAST == 1) {
		if (b < B) tick_fast1_loads<BAKED, Payload>(P, with_comp, fb_counts, fb_list, parity, b);
		return;
	}
	__shared__ real img[StageLayout<FAST, true>::DOUBLES];
	tick_fast_body<FAST, BAKED, Payload>(Pp, with_comp, fb_counts, fb_list, parity, img);
}

#endif	// SAI2B_N == 7

// One task driven on its own, the reference's plugin interface (TemplateTask.h:42-88):
//   updateTaskModel(N_prec)            -> do_torque = 0: the task's nullspace N and N * N_prec; the once-per-
//                                         update singularity bookkeeping when commit_sh
//   computeTorques() / (tau_prec)      -> do_torque = 1: the task's own torques (tau_prec == NULL: the
//                                         no-argument form, no compensation of the previous tasks)
// Nprec_in == NULL is the identity (a task constructed and never given one, JointTask.cpp:62,
// MotionForceTask.cpp:138). Nothing is known about the tasks above, so the range decisions always take
// the Jacobi SVD (the introspection instantiation of the task functions), and a JointTask applies the
// compensation term also behind an identity N_prec, as JointTask::computeTorques(tau_prec) does
// (JointTask.cpp:285-292). Used for examples 01 / 04 / 18-style manual hierarchies; the batched hot path is
// the fused tick above.
// tk_count != NULL: the pass behind task_cert_kernel (sai2b_cert.hip) over the robots it declined, compacted.
__global__ __launch_bounds__(64) void task_kernel(const DevParams* __restrict__ Pp, int task, const double* __restrict__ Nprec_in,
													 const double* __restrict__ tau_prec, double* __restrict__ tau_out,
													 double* __restrict__ N_out, double* __restrict__ Ntot_out, int commit_sh,
													 int do_torque, const int* __restrict__ tk_count, const int* __restrict__ tk_list) {
	const DevParams& P = *Pp;
	const int B = P.B;
	int b = blockIdx.x * 64 + threadIdx.x;
	if (tk_count) {
		if (b >= *(const gint*)tk_count) return;
		b = ((const gint*)tk_list)[b];
	}
	if (b >= B) return;
	RobotCtx rc;
	UNROLL for (int i = 0; i < N; i++) {
		rc.q[i] = ld(P.q, i, B, b);
		rc.dq[i] = ld(P.dq, i, B, b);
	}
	const DevTask& tk = P.task[task];
	{
		Frames F;
		fk(P.model, rc.q, F);
		real M[N * N];
		if (P.payload) {  // wave-uniform
			Payload pl;
			payload_load(P.payload, P.payload_link, B, b, pl);
			mass_matrix(P.model, F, M, pl);
		} else
			mass_matrix(P.model, F, M);
		spd_inverse<N>(M, rc.Minv);
		if (tk.decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES) {
			UNROLL for (int i = 0; i < N; i++) M[i * N + i] = fmax(M[i * N + i], tk.bie_threshold);
			spd_inverse<N>(M, rc.MinvB);
		} else {
			UNROLL for (int i = 0; i < N * N; i++) rc.MinvB[i] = rc.Minv[i];
		}
	}
	real Nprec[N * N], tau[N], tp[N];
	UNROLL for (int i = 0; i < N * N; i++) Nprec[i] = Nprec_in ? ld(Nprec_in, i, B, b) : ((i % (N + 1) == 0) ? 1.0 : 0.0);
	UNROLL for (int i = 0; i < N; i++) tau[i] = tp[i] = tau_prec ? ld(tau_prec, i, B, b) : 0.0;
	Chain chain;
	chain.ok = false;
	chain.wrows = 0;
	UNROLL for (int i = 0; i < N * N; i++) chain.W[i] = 0;
	if (tk.type == SAI2B_MOTION_FORCE_TASK)
		mft_task<true>(P, tk, rc, B, b, false, false, commit_sh != 0, do_torque != 0, Nprec, tau, chain, N_out);
	else
		jt_task<true>(P, tk, rc, B, b, false, false, tau_prec != nullptr, do_torque != 0, Nprec, tau, chain, N_out);
	if (Ntot_out) {
		UNROLL for (int i = 0; i < N * N; i++) st(Ntot_out, i, B, b, Nprec[i]);
	}
	if (do_torque && tau_out) {
		UNROLL for (int i = 0; i < N; i++) st(tau_out, i, B, b, tau[i] - tp[i]);
	}
}

// RobotController::reinitializeTasks (RobotController.cpp:76-80) for every robot: reinit_robot (sai2b_device.hpp)
__global__ __launch_bounds__(64) void reinit_kernel(const DevParams* __restrict__ Pp, int only_task) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	real q[N];
	UNROLL for (int i = 0; i < N; i++) q[i] = ld(P.q, i, B, b);
	reinit_robot(P, only_task, q, B, b);
}

// the SVD-free first kernel of `form`
static int launch_fast(const DevParams* d_params, int B, const TickForm& form, bool with_comp, const WorkList& fb, hipStream_t stream) {
	if (form.fast >= 3) return launch_tick_cert(d_params, B, form, with_comp, fb, stream);	// general hierarchies (sai2b_cert.hip)
#if SAI2B_N == 7
	// [payload][FAST - 1][BAKED]
	static constexpr decltype(&tick_fast_kernel<1, false>) kernel[2][2][2] = {
		{{tick_fast_kernel<1, false>, tick_fast_kernel<1, true>}, {tick_fast_kernel<2, false>, tick_fast_kernel<2, true>}},
		{{tick_fast_payload_kernel<1, false>, tick_fast_payload_kernel<1, true>},
		 {tick_fast_payload_kernel<2, false>, tick_fast_payload_kernel<2, true>}}};
	hipLaunchKernelGGL(kernel[form.payload][form.fast == 2][form.baked], dim3((B + 63) / 64), dim3(64), 0, stream, d_params,
					   with_comp ? 1 : 0, fb.counts, fb.list, fb.parity);
#endif
	return launch_result();
}

// the generic kernel: over the work list fb_count / fb_list (or, NULL, the whole batch), `group` lanes per robot
// report: where the pass over a work list tells the host the list's counts, when the call asks (TickCall::stamp)
static int launch_generic(const DevParams* d_params, int B, const TickCall& call, const int* fb_count, const int* fb_list, hipStream_t stream,
						  unsigned long long* report = nullptr) {
	if (call.group && !call.debug)
		return launch_tick_group(d_params, B, call.group, false, call.commit_sh, call.with_comp, call.do_torque, fb_count, fb_list, stream,
								 call.stamp ? report : nullptr, call.stamp);
	auto* kernel = call.debug ? tick_kernel<true> : tick_kernel<false>;
	hipLaunchKernelGGL(kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_params, call.commit_sh ? 1 : 0, call.with_comp ? 1 : 0,
					   call.do_torque ? 1 : 0, fb_count, fb_list);
	return launch_result();
}

int launch_tick(const DevParams* d_params, int B, const TickForm& form, const TickCall& call, const WorkList& fb, hipStream_t stream) {
	// the fast path produces torques only: introspection and model-only passes use the generic kernel
	if (call.debug || form.fast == 0 || !call.do_torque || !call.commit_sh) return launch_generic(d_params, B, call, nullptr, nullptr, stream);
	if (form.self) return launch_tick_self(d_params, B, form, call.with_comp, fb, call.stamp, stream);
	const int rc = launch_fast(d_params, B, form, call.with_comp, fb, stream);
	return launch_generic(d_params, B, call, fb.count(), fb.list, stream, fb.report) | rc;
}

// the range pass of hierarchies with gated generators (same DEBUG variant as the tick that follows, so that
// both take the same range decisions)
int launch_range_pass(const DevParams* d_params, int B, bool debug, bool with_comp, int group, hipStream_t stream) {
	if (!debug && group) return launch_tick_group(d_params, B, group, true, false, with_comp, false, nullptr, nullptr, stream);
	auto* kernel = debug ? tick_kernel<true, true> : tick_kernel<false, true>;
	hipLaunchKernelGGL(kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_params, 0, with_comp ? 1 : 0, 0, nullptr, nullptr);
	return launch_result();
}

int launch_tick_part(const DevParams* d_params, int B, const TickForm& form, bool debug, int part, const WorkList& fb, int group,
					 hipStream_t stream) {
	TickCall call;
	call.debug = debug, call.group = group;
	if (debug || form.fast == 0) return launch_generic(d_params, B, call, nullptr, nullptr, stream);
	if (part == 1) return launch_generic(d_params, B, call, fb.count(), fb.list, stream);
	if (form.self) return launch_tick_self(d_params, B, form, true, fb, 0, stream);
	return launch_fast(d_params, B, form, true, fb, stream);
}

int launch_reinit(const DevParams* d_params, int B, int only_task, hipStream_t stream) {
	hipLaunchKernelGGL(reinit_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_params, only_task);
	return launch_result();
}

int launch_task(const DevParams* d_params, int B, int task, const double* Nprec_in, const double* tau_prec, double* tau_out, double* N_out,
				double* Ntot_out, bool commit_sh, bool do_torque, const int* tk_count, const int* tk_list, hipStream_t stream) {
	hipLaunchKernelGGL(task_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_params, task, Nprec_in, tau_prec, tau_out, N_out, Ntot_out,
					   commit_sh ? 1 : 0, do_torque ? 1 : 0, tk_count, tk_list);
	return launch_result();
}

}  // namespace sai2b

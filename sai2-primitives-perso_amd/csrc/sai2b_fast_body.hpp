// sai2b_fast_body.hpp — the per-lane body of the SVD-free headline kernels, shared by the two forms of the tick:
// tick_fast_kernel (sai2b_kernels.hip: declined robots go to the work list of the generic kernel launched behind) and
// tick_self_kernel (sai2b_self.hip: SELF, a wavefront serves its own declined robots, no launch behind).
#pragma once
#include <hip/hip_runtime.h>

#include "sai2b_device.hpp"
#include "sai2b_fast.hpp"
#include "sai2b_baked_panda.h"
#include "sai2b_baked_panda_model.h"

namespace sai2b {

#if SAI2B_N == 7  // the SVD-free kernels are for 7-joint robots (6-DOF task + a one-dimensional nullspace)
// The model phase of the BAKED kernels: overloads on PandaBaked that the calls below take in place of the generic templates
// of sai2b_device.hpp. They run the generated straight-line forms (sai2b_baked_panda_model.h), which keep only the nonzero
// terms of the Panda's constants; the payload forms keep payload_terms() and their selects as the generic ones have them.
DI void fk(const PandaBaked&, const real* q, Frames& F) {
	real sn[N], cs[N];
	UNROLL for (int i = 0; i < N; i++) sincos_joint(q[i], &sn[i], &cs[i]);
	panda_fk(sn, cs, F);
}
DI void jacobian(const PandaBaked&, const DevTask& t, const Frames& F, const real* x, real* J) { panda_jacobian(F, t.link, x, J); }
DI void jacobian(const PandaBaked&, const FastPose& t, const Frames& F, const real* x, real* J) { panda_jacobian(F, t.link, x, J); }
DI void mass_matrix(const PandaBaked&, const Frames& F, real* M, const NoPayload& = NoPayload{}) { panda_mass_matrix(F, M); }
DI void mass_matrix(const PandaBaked&, const Frames& F, real* M, const Payload& pl) {
	PayloadTerms pt;
	payload_terms(pl, F, pt);
	panda_mass_matrix_payload(F, pl.link, pt, M);
}
DI void gravity_vector(const PandaBaked&, const Frames& F, real* g, const NoPayload& = NoPayload{}) { panda_gravity_vector(F, g); }
DI void gravity_vector(const PandaBaked&, const Frames& F, real* g, const Payload& pl) {
	PayloadTerms pt;
	payload_terms(pl, F, pt);
	panda_gravity_vector_payload(F, pl.link, pt, g);
}

// M and g of the headline kernels' model phase. PL = NoPayload: the code this was before payloads existed.
template <bool BAKED, class PL>
DI void fast_model(const DevParams& P, const Frames& F, const PL& pl, real* M, real* g) {
	if constexpr (BAKED)
		mass_matrix(PandaBaked{}, F, M, pl);
	else
		mass_matrix(P.model, F, M, pl);
	if (P.gravity_comp) {
		if constexpr (BAKED)
			gravity_vector(PandaBaked{}, F, g, pl);
		else
			gravity_vector(P.model, F, g, pl);
	}
	else {
		UNROLL for (int i = 0; i < N; i++) g[i] = 0;
	}
}
// the same with gravity compensation as a bit of the FastBlock's flags word (FAST = 2)
template <bool BAKED, class PL>
DI void fast_model(const DevParams& P, bool gravity_comp, const Frames& F, const PL& pl, real* M, real* g) {
	if constexpr (BAKED)
		mass_matrix(PandaBaked{}, F, M, pl);
	else
		mass_matrix(P.model, F, M, pl);
	if (gravity_comp) {
		if constexpr (BAKED)
			gravity_vector(PandaBaked{}, F, g, pl);
		else
			gravity_vector(P.model, F, g, pl);
	}
	else {
		UNROLL for (int i = 0; i < N; i++) g[i] = 0;
	}
}

// Where a lane learns whether its robot stays on the SVD-free path. true: it does not, the lane touches no state and leaves
// the body. Two launches: the robot is appended to the work list (worklist_append, which also keeps the largest number of
// declined robots of one wavefront in fb_counts[4 + parity], what the host needs to choose the self form again). SELF: nothing
// is written here, the kernel takes the ballot once every lane is back (tick_self_kernel).
template <bool SELF>
DI bool fast_declined(int* __restrict__ fb_counts, int* __restrict__ fb_list, int parity, bool mine, int b) {
	if constexpr (SELF)
		return !mine;
	else
		return worklist_append(fb_counts, fb_list, parity, mine, b, fb_counts + 4);
}

// [full MFT] (FAST = 1) with its inputs loaded into registers up front, as before the staged path: at C2's 4 096
// robots (one wavefront per 16 SIMDs, nothing to contend for HBM) the staged form measured 13 % slower.
// Returns whether the robot was declined.
template <bool BAKED, class PL, bool SELF = false>
DI bool tick_fast1_loads(const DevParams& P, int with_comp, int* __restrict__ fb_counts, int* __restrict__ fb_list, int parity,
						 int b) {
	const int B = P.B;
	RobotCtx rc;
	UNROLL for (int i = 0; i < N; i++) {
		rc.q[i] = ld(P.q, i, B, b);
		rc.dq[i] = ld(P.dq, i, B, b);
	}
	const DevTask& t0 = P.task[0];
	const bool clean = ldi(t0.istate, IS_NTYPES, B, b) == 0;
	// Phase order keeps the live set small and gives every load a phase of arithmetic to hide behind:
	// FK/Jacobian -> MFT law -> CRBA -> certificate.
	JtEarly jt;
	MftIn in0;
	mft_load(t0, B, b, in0);
	SAI2B_PHASE();
	real J[6 * N], M[N * N], g[N], Fu[6], Ff[6];
	{
		Frames F;
		if constexpr (BAKED)
			fk(PandaBaked{}, rc.q, F);
		else
			fk(P.model, rc.q, F);
		real x[3], R[9];
		frame_pose(t0, F, x, R);
		if constexpr (BAKED)
			jacobian(PandaBaked{}, t0, F, x, J);
		else
			jacobian(P.model, t0, F, x, J);
		SAI2B_PHASE();
		mft_law(t0, rc, J, x, R, in0, Fu, Ff);	// MotionForceTask.cpp:278-503 (integrators not yet stored)
		SAI2B_PHASE();
		if constexpr (PL::on) {	 // (the ten rows are loaded here, not with the other inputs: nothing of them is live across the law)
			PL pl;
			payload_load(P.payload, P.payload_link, B, b, pl);
			fast_model<BAKED>(P, F, pl, M, g);
		} else {	// spelled out as it was before payloads: the register allocation of this form follows the text
			if constexpr (BAKED)
				mass_matrix(PandaBaked{}, F, M);
			else
				mass_matrix(P.model, F, M);
			if (P.gravity_comp) {
				if constexpr (BAKED)
					gravity_vector(PandaBaked{}, F, g);
				else
					gravity_vector(P.model, F, g);
			}
			else {
				UNROLL for (int i = 0; i < N; i++) g[i] = 0;
			}
		}
	}
	SAI2B_PHASE();
	const bool ok = certify_nonsingular(J, t0.s_abs_tol, t0.s_max);
	const bool mine = ok && clean;
	if (fast_declined<SELF>(fb_counts, fb_list, parity, mine, b)) return true;
	mft_store_integrators(t0, B, b, in0);
	SAI2B_PHASE();
	real tau[N];
	JtGiven none{jt};
	fast_tick<false>(P, J, M, Fu, Ff, B, b, with_comp != 0, none, tau);
	UNROLL for (int i = 0; i < N; i++) st(P.tau, i, B, b, tau[i] + g[i]);
	return false;
}

// FAST = 1: hierarchy [full MFT]; FAST = 2: [full MFT, full JT] — the SVD-free path of
// sai2b_fast.hpp. A robot takes it only when it is certified non-singular (and is not leaving a
// singular region); otherwise its lane touches no state and appends the robot to the work list of
// the generic kernel launched right behind (one atomic per wavefront that has such robots).
// fb_counts: two counters alternating between ticks (`parity`): this launch fills [parity] and clears
// [1 - parity] for the next one (the generic pass that read it finished before this kernel started).
// BAKED selects where the robot constants come from: false = the ctx's parameter block (any robot),
// true = the stock Panda (chosen by the host only when the ctx model is bit-equal to sai2b_baked_panda.h): the model
// phase is the straight-line code of sai2b_baked_panda_model.h, written out at build time from the nonzero terms of those
// constants (the PandaBaked overloads at the top of this file), with no loads from the parameter block.
// PL = Payload: the form for contexts with per-robot payloads (tick_fast_payload_kernel); its ten rows join the staged
// image (StageLayout<FAST, true>), so nothing of them is live, and no global load is issued, before the model phase reads
// them from LDS. img: the kernel's LDS image.
// Returns whether the robot was declined (fast_declined above). SELF: lanes past the batch come back too (not declined), so
// that the whole wavefront reaches the caller's ballot.
template <int FAST, bool BAKED, class PL, bool SELF = false>
DI bool tick_fast_body(const DevParams* __restrict__ Pp, int with_comp, int* __restrict__ fb_counts, int* __restrict__ fb_list,
					   int parity, real* img) {
	const DevParams& P = *Pp;
	// Batch-uniform parameters: from the FastBlock (sai2b_params.h), one group per phase, each fetched as one burst of wide
	// scalar loads behind one wait. Only the robot constants of the !BAKED forms are still read where DevParams keeps them.
	const FastBlock& fb = P.fast;
	// entry: B and the row bases of q and of the image (first line of the group), in registers before q is asked for and before
	// the first DMA instruction
	FastEntry e = fb.entry;
	sgpr_tie(e.B), sgpr_tie(e.q), sgpr_tie(e.dq), sgpr_tie(e.law_goals0), sgpr_tie(e.state0), sgpr_tie(e.istate0);
	if constexpr (PL::on) sgpr_tie(e.payload), sgpr_tie(e.law_goals1), sgpr_tie(e.state1);  // (rows of the payload forms' image)
	const int B = e.B;
	const int b0 = blockIdx.x * 64, b = b0 + threadIdx.x;
	// Inputs: q in registers (FK needs it and nothing else), every other row by DMA into the LDS image (StageLayout,
	// sai2b_fast.hpp). q is waited for before the DMA is issued, and the window up to the barrier issues no other
	// global load and touches no scratch, so the DMA lands behind the kinematics and the barrier retires it.
	using S = StageLayout<FAST, PL::on>;
	RobotCtx rc;
	UNROLL for (int i = 0; i < N; i++) rc.q[i] = ld(e.q, i, B, min(b, B - 1));
	// the wait for q goes here, ahead of the DMA: one wait, behind the last of the seven loads
	UNROLL for (int i = 0; i < N; i++) asm volatile("" : "+v"(rc.q[i]));
	SAI2B_PHASE();
	stage_issue<FAST, PL::on>(e, img, b0);
	SAI2B_PHASE();
	if (b >= B) return false;
	const DevTask& t0 = P.task[0];
	const real* col = img + threadIdx.x;
	// Window: FK -> frame pose -> Jacobian -> (CRBA, gravity) -> certificate, from q alone. Without payload the model
	// phase runs here, while the frames are alive anyway, and parks M and g in this lane's column of the rows behind
	// the DMA image (S::PARKED): neither is live in registers across the certificate or the control law, and no
	// barrier is owed for them (a lane reads back only what it wrote). The payload form's CRBA needs rows the DMA
	// brings, so it keeps the model phase behind the law and evaluates FK a second time there.
	real J[6 * N], x[3], R[9];
	real s_abs_tol, s_max;
	{
		Frames F;
		// pose and certificate group. BAKED: asked for ahead of FK, which hides its one round trip, and pinned behind it.
		// Otherwise read where it lies, value by value: FK and the CRBA stream the robot constants through the scalar
		// registers and have none to spare for values they do not use.
		if constexpr (BAKED) {
			FastPose pose = fb.pose;
			fk(PandaBaked{}, rc.q, F);
			UNROLL for (int k = 0; k < 3; k++) sgpr_tie(pose.frame_pos[k]);
			UNROLL for (int k = 0; k < 9; k++) sgpr_tie(pose.frame_rot[k]);
			sgpr_tie(pose.link), sgpr_tie(pose.s_abs_tol), sgpr_tie(pose.s_max);
			s_abs_tol = pose.s_abs_tol, s_max = pose.s_max;
			frame_pose(pose, F, x, R);
			jacobian(PandaBaked{}, pose, F, x, J);
		} else {
			fk(P.model, rc.q, F);
			frame_pose(fb.pose, F, x, R);
			jacobian(P.model, fb.pose, F, x, J);
		}
		if constexpr (S::PARKED) {
			SAI2B_PHASE();
			real M[N * N], g[N];
			// (the flags word is asked for behind the window: across it, it would be one more value held in a scalar register;
			// the !BAKED forms, which read the robot constants where DevParams keeps them, take the flag from there too)
			fast_model<BAKED>(P, BAKED ? (fb.entry.flags & FB_GRAVITY_COMP) != 0 : P.gravity_comp != 0, F, PL{}, M, g);
			real* park = img + S::IMAGE + threadIdx.x;
			UNROLL for (int i = 0; i < N; i++) UNROLL for (int j = 0; j <= i; j++) park[(i * (i + 1) / 2 + j) * 64] = M[i * N + j];
			UNROLL for (int i = 0; i < N; i++) park[(S::MROWS + i) * 64] = g[i];
		}
	}
	SAI2B_PHASE();
	if constexpr (!BAKED) s_abs_tol = fb.pose.s_abs_tol, s_max = fb.pose.s_max;
	const bool ok = certify_nonsingular(J, s_abs_tol, s_max);
	SAI2B_PHASE();
	// the flags word of everything behind the barrier, the batch size once more (Bp: asked for again, the row stride made from
	// the entry's B would be one more value held, or spilled and fetched back, across the window) and the law's group: asked
	// for ahead of the barrier, behind whose waits they arrive
	int flags = fb.entry.flags, Bp = fb.entry.B;
	FastLaw law = fb.law;
	__syncthreads();  // one wavefront per workgroup: vmcnt(0) + barrier, the DMA-written image is readable from here
	sgpr_tie(flags), sgpr_tie(Bp);
	UNROLL for (int i = 0; i < N; i++) {
		rc.dq[i] = col[(S::DQ + i) * 64];
		if constexpr (!S::PARKED) rc.q[i] = ld(e.q, i, Bp, b);  // again (an L2 hit): not live across the window
	}
	const bool clean = ((const int*)(img + S::IROW * 64))[threadIdx.x] == 0;
	MftIn in0;
	fast_mft_load(flags, StagedRows{t0, Bp, b, col + S::MG * 64, col + S::MS * 64, 6}, in0);
	SAI2B_PHASE();
	real Fu[6], Ff[6];
	// MotionForceTask.cpp:278-503 (integrators not yet stored)
	real v[3], w[3];  // J dq (MotionForceTask.cpp:293-298)
	mv<3, N>(J, rc.dq, v);
	mv<3, N>(J + 3 * N, rc.dq, w);
	if (flags & FB_PLAIN_MOTION) {
		sgpr_tie(law.dt);
		UNROLL for (int k = 0; k < 3; k++) {
			sgpr_tie(law.kp_pos[k]), sgpr_tie(law.kv_pos[k]), sgpr_tie(law.ki_pos[k]);
			sgpr_tie(law.kp_ori[k]), sgpr_tie(law.kv_ori[k]), sgpr_tie(law.ki_ori[k]);
		}
		fast_mft_law_plain(law, v, w, x, R, in0, Fu, Ff);
	} else {
		mft_law_vw(t0, v, w, x, R, in0, Fu, Ff);  // any other task: the law as the generic kernels have it
	}
	// second line of the entry group
	e.tau = fb.entry.tau, e.law_goals1 = fb.entry.law_goals1, e.state1 = fb.entry.state1;
	e.q_again = fb.entry.q_again, e.state0_again = fb.entry.state0_again;
	SAI2B_PHASE();
	real tau[N];
	if constexpr (S::PARKED) {
		const bool mine = ok && clean;
		if (fast_declined<SELF>(fb_counts, fb_list, parity, mine, b)) return true;
		sgpr_tie(e.tau), sgpr_tie(e.law_goals1), sgpr_tie(e.state1), sgpr_tie(e.q_again), sgpr_tie(e.state0_again);
		fast_mft_store_integrators(flags, e.state0_again, Bp, b, in0);  // committed to the fast path: integrators can go out now
		SAI2B_PHASE();
		// the JointTask law and its integrator store are the chain's, behind the nullspace vector (JtLate)
		const real* park = col + S::IMAGE;
		JtLate<BAKED> jt{fb.jt, (flags & FB_JT_VSAT) != 0, e.law_goals1, e.state1, Bp, b, col + S::DQ * 64, e.q_again};
		fast_tick2(flags, fb.chain, J, LdsSym{park}, Fu, Ff, with_comp != 0, jt, tau);
		UNROLL for (int i = 0; i < N; i++) st(e.tau, i, Bp, b, tau[i] + park[(S::MROWS + i) * 64]);
	} else {
		real M[N * N], g[N];
		{
			PL pl;
			if constexpr (PL::on) {
				pl.link = fb.entry.payload_link;
				pl.m = col[S::PLD * 64];
				UNROLL for (int k = 0; k < 3; k++) pl.c[k] = col[(S::PLD + 1 + k) * 64];
				UNROLL for (int k = 0; k < 6; k++) pl.I[k] = col[(S::PLD + 4 + k) * 64];
			}
			Frames F;
			if constexpr (BAKED)
				fk(PandaBaked{}, rc.q, F);
			else
				fk(P.model, rc.q, F);
			fast_model<BAKED>(P, (flags & FB_GRAVITY_COMP) != 0, F, pl, M, g);
		}
		SAI2B_PHASE();
		const bool mine = ok && clean;
		if (fast_declined<SELF>(fb_counts, fb_list, parity, mine, b)) return true;
		sgpr_tie(e.tau), sgpr_tie(e.state1), sgpr_tie(e.state0_again);
		// the JointTask law, from its staged rows (late: its results would be live across the model phase)
		JtEarly je;
		if constexpr (FAST == 2)
			fast_jt_early(fb.jt, (flags & FB_JT_VSAT) != 0, rc, StagedRows{P.task[1], Bp, b, col + S::JG * 64, col + S::JS * 64, N}, je);
		// committed to the fast path: integrators can go out now
		fast_mft_store_integrators(flags, e.state0_again, Bp, b, in0);
		if (FAST == 2) {
			UNROLL for (int i = 0; i < N; i++) st(e.state1, i, Bp, b, je.integ[i]);
		}
		SAI2B_PHASE();
		JtGiven jt{je};
		if constexpr (FAST == 2)
			fast_tick2(flags, fb.chain, J, M, Fu, Ff, with_comp != 0, jt, tau);
		else
			fast_tick<false>(P, J, M, Fu, Ff, Bp, b, with_comp != 0, jt, tau);
		UNROLL for (int i = 0; i < N; i++) st(e.tau, i, Bp, b, tau[i] + g[i]);
	}
	return false;
}
#endif	// SAI2B_N == 7

}  // namespace sai2b

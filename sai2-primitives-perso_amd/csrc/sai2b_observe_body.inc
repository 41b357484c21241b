// sai2b_observe_body.inc — the one text of observe_kernel and observe_reward_kernel, included twice by sai2b_observe.hip with
// OBSERVE_REWARD 0 and 1 (REW_OR(x): nothing, or || (x)). A preprocessor switch and not a template: with OBSERVE_REWARD 0 the
// compiler sees observe_kernel's text as it was before the reward existed, so its instructions are the same by construction.
#if OBSERVE_REWARD
__global__ __launch_bounds__(64) void observe_reward_kernel(const DevParams* __restrict__ Pp, const ObsParams O, const RewParams W,
															 real* __restrict__ out, unsigned char* __restrict__ done,
															 int* __restrict__ steps, int* __restrict__ counts) {
#else
__global__ __launch_bounds__(64) void observe_kernel(const DevParams* __restrict__ Pp, const ObsParams O, real* __restrict__ out,
													  unsigned char* __restrict__ done, int* __restrict__ steps, int* __restrict__ counts) {
#endif
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
	// ---- reward: the global terms that need no kinematics. tau is read in any case: it becomes the next call's tau_prev.
#if OBSERVE_REWARD
	real rew_tau[N], rew_speed = 0, rew_torque = 0, rew_rate = 0, rew_limit = 0;
	{
		UNROLL for (int i = 0; i < N; i++) rew_tau[i] = ld(P.tau, i, B, b);
		if (W.terms & SAI2B_REW_JOINT_SPEED) {
			UNROLL for (int i = 0; i < N; i++) rew_speed += dq[i] * dq[i];
			if (W.rows) st(W.rows, W.row_global[1], B, b, rew_speed);
		}
		if (W.terms & SAI2B_REW_TORQUE) {
			UNROLL for (int i = 0; i < N; i++) rew_torque += rew_tau[i] * rew_tau[i];
			if (W.rows) st(W.rows, W.row_global[2], B, b, rew_torque);
		}
		if (W.terms & SAI2B_REW_TORQUE_RATE) {
			if (ldi(W.episode, 1, B, b)) {
				UNROLL for (int i = 0; i < N; i++) {
					const real d = rew_tau[i] - ld(W.state, REW_TAU_PREV + i, B, b);
					rew_rate += d * d;
				}
			}
			if (W.rows) st(W.rows, W.row_global[3], B, b, rew_rate);
		}
		if (W.terms & SAI2B_REW_LIMIT) {
			rew_limit = fmax(0.0, W.limit_soft_margin - margin);
			if (W.rows) st(W.rows, W.row_global[4], B, b, rew_limit);
		}
		if ((W.terms & SAI2B_REW_ALIVE) && W.rows) st(W.rows, W.row_global[0], B, b, 1.0);
	}
#endif
	// ---- tasks: observed ones, and those a criterion (or a reward term) reads
	const int success_mask = (O.criteria & SAI2B_DONE_SUCCESS) ? O.success_mask : 0;
	const int force_mask = (O.criteria & SAI2B_DONE_FORCE) ? O.force_mask : 0;
	const int stored_mask = out ? O.task_mask : 0;
#if OBSERVE_REWARD
	const int visit_mask = (stored_mask && O.task_blocks ? stored_mask : 0) | success_mask | force_mask | (W.task_terms ? W.task_mask : 0);
#else
	const int visit_mask = (stored_mask && O.task_blocks ? stored_mask : 0) | success_mask | force_mask;
#endif
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
			// reward: this task's terms, its first term row, and a lane's cell of that row in rew_task_terms
#if OBSERVE_REWARD
			const int rt = ((W.task_mask >> k) & 1) ? W.task_terms : 0, rrow = W.row_task[k];
			auto task_term = [&](int bit, real v) {
				const int r = rrow + W.off_task[bit];
				rew_task_terms[(r - W.global_rows) * 64 + threadIdx.x] = v;
				if (W.rows) st(W.rows, r, B, b, v);
			};
#endif
			real x[3], R[9];
			frame_pose(t, F, x, R);
			if (tb & SAI2B_OBS_POSE) {
				UNROLL for (int a = 0; a < 3; a++) st(out, row + a, B, b, x[a]);
				UNROLL for (int a = 0; a < 9; a++) st(out, row + 3 + a, B, b, R[a]);
				row += OBS_POSE_ROWS;
			}
			if ((tb & SAI2B_OBS_TWIST) REW_OR(rt & REW_NEED_TWIST)) {
				real J[6 * N], v[6];
				jacobian(P.model, t, F, x, J);
				mv<6, N>(J, dq, v);
#if OBSERVE_REWARD
				if (tb & SAI2B_OBS_TWIST) {
					UNROLL for (int a = 0; a < 6; a++) st(out, row + a, B, b, v[a]);
					row += OBS_TWIST_ROWS;
				}
				if (rt & SAI2B_REW_LIN_VEL_SQ) task_term(REW_BIT_LIN_VEL_SQ, v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
				if (rt & SAI2B_REW_ANG_VEL_SQ) task_term(REW_BIT_ANG_VEL_SQ, v[3] * v[3] + v[4] * v[4] + v[5] * v[5]);
#else
				UNROLL for (int a = 0; a < 6; a++) st(out, row + a, B, b, v[a]);
				row += OBS_TWIST_ROWS;
#endif
			}
			// reward: sigma_f of this task where the error block has computed it (FORCE_ERR_SQ reads it below)
#if OBSERVE_REWARD
			real rew_sf[9];
			bool rew_have_sf = false;
#endif
			const bool for_success = (success_mask >> k) & 1;
			if ((tb & SAI2B_OBS_ERROR) || for_success REW_OR(rt & REW_NEED_ERROR)) {
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
#if OBSERVE_REWARD
				{
					if (rt & SAI2B_REW_POS) task_term(REW_BIT_POS, pn);
					if (rt & SAI2B_REW_POS_SQ) task_term(REW_BIT_POS_SQ, pn * pn);
					if (rt & SAI2B_REW_POS_TANH) task_term(REW_BIT_POS_TANH, 1.0 - tanh(pn / W.pos_scale[k]));
					if (rt & SAI2B_REW_ORI) task_term(REW_BIT_ORI, on);
					if (rt & SAI2B_REW_ORI_SQ) task_term(REW_BIT_ORI_SQ, on * on);
					if (rt & SAI2B_REW_ORI_TANH) task_term(REW_BIT_ORI_TANH, 1.0 - tanh(on / W.ori_scale[k]));
					UNROLL for (int a = 0; a < 9; a++) rew_sf[a] = sf[a];
					rew_have_sf = true;
				}
#endif
			}
			const bool for_force = (force_mask >> k) & 1;
			if ((tb & SAI2B_OBS_SENSED) || for_force REW_OR(rt & REW_NEED_SENSED)) {
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
#if OBSERVE_REWARD
				{
					if (rt & SAI2B_REW_FORCE_ERR_SQ) {
						if (!rew_have_sf) {	 // uniform: the error block was not needed for this task
							real sp[9];
							sigma_pair(t, 0, t.fdim, t.faxis, R, rew_sf, sp);
						}
						real df[3], sdf[3];
						UNROLL for (int a = 0; a < 3; a++) df[a] = fs_w[a] - ld(t.goals, MFT_GOAL_FORCE + a, B, b);
						mv3(rew_sf, df, sdf);
						task_term(REW_BIT_FORCE_ERR_SQ, sdf[0] * sdf[0] + sdf[1] * sdf[1] + sdf[2] * sdf[2]);
					}
					if (rt & SAI2B_REW_FORCE_EXCESS)
						task_term(REW_BIT_FORCE_EXCESS,
								  fmax(0.0, sqrt(fs_w[0] * fs_w[0] + fs_w[1] * fs_w[1] + fs_w[2] * fs_w[2]) - W.force_soft_limit[k]));
				}
#endif
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
	// ---- reward: the DONE term, the sum in layout order, the accumulators
#if OBSERVE_REWARD
	{
		real rew = 0.0;
		if (W.terms & SAI2B_REW_ALIVE) rew = rew_mul_add(rew, W.weight[0], 1.0);
		if (W.terms & SAI2B_REW_JOINT_SPEED) rew = rew_mul_add(rew, W.weight[1], rew_speed);
		if (W.terms & SAI2B_REW_TORQUE) rew = rew_mul_add(rew, W.weight[2], rew_torque);
		if (W.terms & SAI2B_REW_TORQUE_RATE) rew = rew_mul_add(rew, W.weight[3], rew_rate);
		if (W.terms & SAI2B_REW_LIMIT) rew = rew_mul_add(rew, W.weight[4], rew_limit);
		if (W.terms & SAI2B_REW_DONE) {
			real dv = 0.0;
			UNROLL for (int r = 0; r < SAI2B_DONE_REASONS; r++) dv += W.done_value[r] * (real)((bits >> r) & 1);
			if (W.rows) st(W.rows, W.row_global[5], B, b, dv);
			rew = rew_mul_add(rew, W.weight[5], dv);
		}
#pragma unroll 1
		for (int s = 0; s < W.task_rows; s++) rew = rew_mul_add(rew, W.row_weight[s], rew_task_terms[s * 64 + threadIdx.x]);
		const bool replaced = !isfinite(rew);
		if (replaced) rew = W.nonfinite_reward;
		if (W.reward) st(W.reward, 0, B, b, rew);
		real ret = rew_mul_add(ld(W.state, REW_RET, B, b), ld(W.state, REW_DISC, B, b), rew);
		real disc = ld(W.state, REW_DISC, B, b) * W.gamma;
		if (bits) {
			st(W.state, REW_LAST_RETURN, B, b, ret);
			sti(W.episode, 0, B, b, step);
			ret = 0.0, disc = 1.0;
		}
		st(W.state, REW_RET, B, b, ret);
		st(W.state, REW_DISC, B, b, disc);
		// tau_prev is written in any case (it is the stored torque of this call) and is valid while the episode goes on
		UNROLL for (int i = 0; i < N; i++) st(W.state, REW_TAU_PREV + i, B, b, rew_tau[i]);
		sti(W.episode, 1, B, b, bits ? 0 : 1);
		const unsigned long long closed = __ballot(bits != 0), bad = __ballot(replaced);
		if (threadIdx.x == 0 && closed) atomicAdd(W.counts + 0, __popcll(closed));
		if (threadIdx.x == 0 && bad) atomicAdd(W.counts + 1, __popcll(bad));
	}
#endif
}

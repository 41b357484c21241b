// sai2b_reset_sampled.inc — reset_sampled_kernel, included by sai2b_otg.hip behind reset_subset_kernel, whose reinit_robot /
// otg_reinit_robot it shares (include/sai2b.h "episode starts" has the law; sai2b_reset_draw.h the draws, shared with the CPU).
//
// One lane per robot, one wavefront per workgroup. A wavefront without a selected robot leaves after its mask load (a uniform
// vote). The try loop: a lane that has accepted waits with its execution bit off; the loop ends when no lane of the wavefront
// is still drawing (a uniform vote per try), so a wavefront pays for its unluckiest robot. One try is ceil(N / 4) Philox calls,
// and, only when a criterion is configured (batch-uniform), fk(), frame_pose() / jacobian() and the one-sided Jacobi of
// sai2b_device.hpp on the N x 6 transpose of P J, whose column norms are the singular values. Everything is FP64 in registers;
// links and tasks are selected with unrolled compares, never by a register index. No LDS.
// The three counts are reduced over the wavefront with shuffles and added by lane 0, one atomic each.

// the singular-value ratio s_(rank-1) / s_0 of P J (criterion (a)); NaN in gives a false comparison at the caller
DI real rs_sv_ratio(const DevTask& t, const real* J) {
	real X[N * 6];	// (P J)^T: X[r][c] = (P J)[c][r]
	if (t.full_projection) {
		UNROLL for (int r = 0; r < N; r++) UNROLL for (int c = 0; c < 6; c++) X[r * 6 + c] = J[c * N + r];
	} else {
		UNROLL for (int r = 0; r < N; r++) UNROLL for (int c = 0; c < 6; c++) {
			real s = 0;
			UNROLL for (int l = 0; l < 6; l++) s = fma(t.P[c * 6 + l], J[l * N + r], s);
			X[r * 6 + c] = s;
		}
	}
	real W[36];
	hestenes<N, 6>(X, W);
	real s2[6];
	UNROLL for (int c = 0; c < 6; c++) {
		real a = 0;
		UNROLL for (int r = 0; r < N; r++) a = fma(X[r * 6 + c], X[r * 6 + c], a);
		s2[c] = a;
	}
	// descending, by a fixed network of compare-exchanges (no indexing by data)
	UNROLL for (int i = 0; i < 5; i++) UNROLL for (int j = 0; j < 5 - i; j++) {
		const real hi = fmax(s2[j], s2[j + 1]), lo = fmin(s2[j], s2[j + 1]);
		s2[j] = hi, s2[j + 1] = lo;
	}
	real sr = s2[0];
	UNROLL for (int k = 1; k < 6; k++)
		if (k == t.rank - 1) sr = s2[k];
	return sqrt(sr) / sqrt(s2[0]);
}

// criteria (a) - (c) on a candidate
DI bool rs_accept(const DevParams& P, const RsParams& S, const real* q, int B, int b) {
	Frames F;
	fk(P.model, q, F);
	bool ok = true;
	if (S.ratio_task >= 0) {
		const DevTask& t = P.task[S.ratio_task];
		real x[3], R[9], J[6 * N];
		frame_pose(t, F, x, R);
		jacobian(P.model, t, F, x, J);
		ok = ok && rs_sv_ratio(t, J) >= S.min_ratio;
	}
	if (S.box_task >= 0) {
		real x[3], R[9];
		frame_pose(P.task[S.box_task], F, x, R);
		UNROLL for (int k = 0; k < 3; k++) ok = ok && x[k] >= S.box_lower[k] && x[k] <= S.box_upper[k];
	}
	if (S.use_clearance) {
		real Rl[9], pl[3];
		UNROLL for (int k = 0; k < 9; k++) Rl[k] = F.R[N - 1][k];
		UNROLL for (int k = 0; k < 3; k++) pl[k] = F.p[N - 1][k];
		UNROLL for (int i = 0; i < N - 1; i++)
			if (P.contact_link == i) {
				UNROLL for (int k = 0; k < 9; k++) Rl[k] = F.R[i][k];
				UNROLL for (int k = 0; k < 3; k++) pl[k] = F.p[i][k];
			}
		real p0[3], nn[3];
		UNROLL for (int k = 0; k < 3; k++) p0[k] = ld(P.contact, k, B, b), nn[k] = ld(P.contact, 3 + k, B, b);
		UNROLL for (int j = 0; j < SAI2B_MAX_CONTACT_POINTS; j++)
			if (j < P.contact_n_points) {
				real d = 0;
				UNROLL for (int k = 0; k < 3; k++) {
					const real xk = fma(Rl[3 * k], P.contact_points[j][0],
										fma(Rl[3 * k + 1], P.contact_points[j][1], fma(Rl[3 * k + 2], P.contact_points[j][2], pl[k])));
					d = fma(nn[k], p0[k] - xk, d);
				}
				ok = ok && d <= -S.clearance;
			}
	}
	return ok;
}

DI int rs_wave_sum(int v) {
	UNROLL for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
	return v;
}

__global__ __launch_bounds__(64) void reset_sampled_kernel(const DevParams* __restrict__ Pp, const RsParams S, const unsigned char* __restrict__ mask,
														   double* __restrict__ q_state, double* __restrict__ dq_state, double* __restrict__ q_pose,
														   int flags) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	const bool selected = b < B && mask[b < B ? b : B - 1] != 0;
	if (!__any(selected)) return;  // wave-uniform
	// (from here on every lane stays to the end: the counts are reduced over the whole wavefront)
	constexpr int CALLS = (N + 3) / 4;
	const unsigned robot = S.rng.first_robot + (unsigned)b, k0 = S.rng.key0, k1 = S.rng.key1;
	unsigned e = 0;
	real lower[4 * CALLS], upper[4 * CALLS], q[4 * CALLS];
	UNROLL for (int i = 0; i < 4 * CALLS; i++) lower[i] = upper[i] = q[i] = 0.0;
	if (selected) {
		e = (unsigned)S.episode[b];
		UNROLL for (int i = 0; i < N; i++) lower[i] = ld(S.rows, i, B, b), upper[i] = ld(S.rows, N + i, B, b);
	}
	const bool criteria = S.ratio_task >= 0 || S.box_task >= 0 || S.use_clearance != 0;	 // batch-uniform
	bool drawing = selected;
	int tries = 0;
#pragma unroll 1
	for (int n = 0; n < S.max_tries; n++) {
		if (!__any(drawing)) break;	 // wave-uniform
		if (drawing) {
			real c[4 * CALLS];
			UNROLL for (int j = 0; j < CALLS; j++) rs_candidate4((unsigned)n, e, (unsigned)j, robot, k0, k1, lower + 4 * j, upper + 4 * j, c + 4 * j);
			bool ok = true;
			UNROLL for (int i = 0; i < N; i++) ok = ok && fabs(c[i]) <= 1.7976931348623157e308;	 // finite
			if (ok && criteria) ok = rs_accept(P, S, c, B, b);
			if (ok) {
				UNROLL for (int i = 0; i < N; i++) q[i] = c[i];
				drawing = false;
				tries = n + 1;
			}
		}
	}
	const bool exhausted = drawing;	 // still drawing after the last try
	real dq[4 * CALLS];
	UNROLL for (int i = 0; i < 4 * CALLS; i++) dq[i] = 0.0;
	if (exhausted) {
		tries = S.max_tries + 1;
		UNROLL for (int i = 0; i < N; i++) q[i] = ld(S.rows, 3 * N + i, B, b);
	}
	real sigma[4 * CALLS];
	bool moving = false;
	UNROLL for (int i = 0; i < 4 * CALLS; i++) sigma[i] = 0.0;
	if (selected && !exhausted) {
		UNROLL for (int i = 0; i < N; i++) {
			sigma[i] = ld(S.rows, 2 * N + i, B, b);
			moving = moving || sigma[i] != 0.0;
		}
	}
	if (__any(moving)) {  // a wavefront whose deviations are all zero does not draw; a lane whose own are zero gets exact zeros
		if (moving) {
			UNROLL for (int j = 0; j < CALLS; j++) rs_velocity4(e, (unsigned)j, robot, k0, k1, sigma + 4 * j, dq + 4 * j);
		}
	}
	if (selected) {
		UNROLL for (int i = 0; i < N; i++) {
			st(q_state, i, B, b, q[i]);
			st(dq_state, i, B, b, dq[i]);
			if (flags & RESET_KEEP_POSE) st(q_pose, i, B, b, q[i]);
			st(P.tau, i, B, b, 0.0);
		}
		reinit_robot(P, -1, q, B, b);
		otg_reinit_robot(P, -1, 0, q, B, b);  // (mode 0 reads the goals reinit_robot has just written, not q)
#pragma unroll 1
		for (int t = 0; t < P.n_tasks; t++) {
			const DevTask& tk = P.task[t];
			if (tk.popc_f) {  // as reset_subset_kernel with RESET_EPISODE
				for (int k = 0; k < 3; k++) st(tk.popc_f, k, B, b, 0.0);
				st(tk.popc_f, 3, B, b, 1.0);  // Rc
				sti(tk.popc_i, 0, B, b, POPC_MAX_COUNTER);
				sti(tk.popc_i, 1, B, b, 0);
				sti(tk.popc_i, 2, B, b, 0);
			}
			// goals: the rows hold the start pose now (this lane wrote them above)
			int row = S.goal_row[0];
			UNROLL for (int k = 1; k < SAI2B_MAX_TASKS; k++)
				if (k == t) row = S.goal_row[k];
			if (!(S.goal_tasks >> t & 1u) || row < 0) continue;
			if (tk.type == SAI2B_MOTION_FORCE_TASK) {
				real u[4], w[4];
				rs_uniforms4((unsigned)t, e, RS_STREAM_GOAL, 0u, robot, k0, k1, u);
				const bool absolute = S.absolute_position >> t & 1u;
				UNROLL for (int k = 0; k < 3; k++) {
					const real p = rs_lerp(ld(S.rows, row + k, B, b), ld(S.rows, row + 3 + k, B, b), u[k]);
					st(tk.goals, MFT_GOAL_POS + k, B, b, absolute ? p : ld(tk.goals, MFT_GOAL_POS + k, B, b) + p);
				}
				const real theta_max = ld(S.rows, row + 6, B, b);
				if (theta_max != 0.0) {
					rs_uniforms4((unsigned)t, e, RS_STREAM_GOAL, 1u, robot, k0, k1, w);
					real axis[3], D[9], R[9], G[9];
					rs_axis_rotation(theta_max * u[3], w[0], w[1], axis, D);
					UNROLL for (int k = 0; k < 9; k++) R[k] = ld(tk.goals, MFT_GOAL_ROT + k, B, b);
					rs_rotate(R, D, G);
					UNROLL for (int k = 0; k < 9; k++) st(tk.goals, MFT_GOAL_ROT + k, B, b, G[k]);
				}
			} else {
				UNROLL for (int j = 0; j < CALLS; j++) {
					if (4 * j >= tk.k0) continue;
					real u[4];
					rs_uniforms4((unsigned)t, e, RS_STREAM_GOAL, (unsigned)j, robot, k0, k1, u);
					UNROLL for (int k = 0; k < 4; k++)
						if (4 * j + k < tk.k0 && 4 * j + k < N)
							st(tk.goals, 4 * j + k, B, b, ld(tk.goals, 4 * j + k, B, b) + rs_joint_offset(ld(S.rows, row + 4 * j + k, B, b), u[k]));
				}
			}
		}
		S.episode[b] = (int)(e + 1u);
		S.tries[b] = tries;
	}
	const int n_reset = rs_wave_sum(selected ? 1 : 0);
	const int n_rejected = rs_wave_sum(selected ? (exhausted ? S.max_tries : tries - 1) : 0);
	const int n_exhausted = rs_wave_sum(exhausted ? 1 : 0);
	if (threadIdx.x == 0) {
		atomicAdd(S.counts + 0, n_reset);
		if (n_rejected) atomicAdd(S.counts + 1, n_rejected);
		if (n_exhausted) atomicAdd(S.counts + 2, n_exhausted);
	}
}

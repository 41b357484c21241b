// sai2b_fast.hpp — SVD-free fast path of the tick for the hierarchies
//     [full 6-DOF MotionForceTask]                        (BASELINE config 2)
//     [full 6-DOF MotionForceTask, full JointTask]        (BASELINE configs 3 and 5)
// taken by a robot only when it carries a certificate that the SingularityHandler's decision is "fully
// non-singular" (SingularityHandler.cpp:100-141). In that
// branch the reference's result does not depend on the singular vectors at all:
//     tau_mft = J^T ( (J Mb^-1 J^T)^-1 F_unit + F_force )            (U_ns cancels, :307-309)
//     N       = I - M^-1 J^T (J M^-1 J^T)^-1 J  =  nv (M nv)^T / (nv^T M nv)   for any nv in null(J)
// (N projects onto null(J), one-dimensional for 7 joints, along range(M^-1 J^T): N = nv c^T with c^T nv = 1 and
// M^-1 c in null(J), so c = M nv / (nv^T M nv)). With a = nv / sqrt(nv^T M nv), b = M a the nullspace projector is the
// rank-one matrix a b^T, a^T M a = 1, and the whole
// second-level JointTask (JointTask.cpp:218-356) collapses to a handful of dot products:
//     Jp = N,  range(Jp) = span(a),  R M_partial R^T = a a^T / |a|^4,
//     R (R^T Jp Mb^-1 Jp^T R)^-1 R^T = a a^T / (beta |a|^4),   beta = b^T Mb^-1 b.
// The singular values themselves are needed only for the branch decision, which is replaced by a
// certificate on G = J J^T:  lambda_max(G) <= ub := tr(G^8)^(1/8) <= 6^(1/8) lambda_max(G), and
// G - s_max^2 ub I positive definite  =>  s_5/s_0 >= s_max (and every s_i/s_0 with it).
// A robot the certificate cannot vouch for (s_5/s_0 below ~0.067, or anything singular) touches no state here
// and is appended to a work list (one atomic per wavefront that has such robots); the generic kernel launched
// right behind runs over that compacted list, so the results are the reference's in all cases.
#pragma once
#include "sai2b_device.hpp"

namespace sai2b {

// Cholesky factor of an SPD n x n matrix: lower L (row-major, upper part untouched) and the
// reciprocals of its diagonal. A is anything indexed [i * n + j] for j <= i (an array, or LdsSym below).
template <int n, class Mat>
DI void chol(const Mat& A, real* L, real* dinv) {
	UNROLL for (int j = 0; j < n; j++) {
		real s = A[j * n + j];
		UNROLL for (int k = 0; k < j; k++) s = fma(-L[j * n + k], L[j * n + k], s);
		real r = rsqrt(s);
		dinv[j] = r;
		L[j * n + j] = s * r;
		UNROLL for (int i = j + 1; i < n; i++) {
			real t = A[i * n + j];
			UNROLL for (int k = 0; k < j; k++) t = fma(-L[i * n + k], L[j * n + k], t);
			L[i * n + j] = t * r;
		}
	}
}
// x <- L^-1 x (forward substitution)
template <int n>
DI void solve_lower(const real* L, const real* dinv, real* x) {
	UNROLL for (int i = 0; i < n; i++) {
		real t = x[i];
		UNROLL for (int k = 0; k < i; k++) t = fma(-L[i * n + k], x[k], t);
		x[i] = t * dinv[i];
	}
}
// x <- L^-T x (back substitution)
template <int n>
DI void solve_lower_t(const real* L, const real* dinv, real* x) {
	UNROLL for (int i = n - 1; i >= 0; i--) {
		real t = x[i];
		UNROLL for (int k = i + 1; k < n; k++) t = fma(-L[k * n + i], x[k], t);
		x[i] = t * dinv[i];
	}
}

// Certificate for "s_0 >= s_abs_tol and s_5 / s_0 >= s_max" on the 6 x 7 Jacobian (see header).
DI bool certify_nonsingular(const real* J, real s_abs_tol, real s_max) {
	real G[36];
	mm_nt_sym<6, N>(J, J, G);
	return certify_gram<6>(G, nullptr, s_abs_tol * s_abs_tol, s_max * s_max);
}

// Inputs of the second-level JointTask law after the early part (fast_jt_early): the PD(+I) unit
// torques f, the goal accelerations, and the advanced integrators (stored once the wavefront is
// committed to the fast path).
struct JtEarly {
	real f[N], ddq[N], integ[N];
};
// A batch-uniform value of the FastBlock, pinned in scalar registers from here on. The reads of a group are written first and
// the ties behind them: every tie needs its value, so the group's scalar loads are all issued ahead of the first tie and one
// wait serves the lot; nothing of the group is fetched again later, one field and one wait at a time.
template <class T>
DI void sgpr_tie(T& v) {
	asm volatile("" : "+s"(v));
}
// Gains of the JointTask law in registers, fetched as one burst. VSAT: with the velocity-saturation limits.
struct JtGains {
	real dt, kp[N], kv[N], ki[N], vsat[N];
};
template <bool VSAT>
DI void jt_gains_burst(const FastJt& s, JtGains& g) {
	g.dt = s.dt;
	UNROLL for (int i = 0; i < N; i++) {
		g.kp[i] = s.kp[i], g.kv[i] = s.kv[i], g.ki[i] = s.ki[i];
		if constexpr (VSAT) g.vsat[i] = s.vsat[i];
	}
	sgpr_tie(g.dt);
	UNROLL for (int i = 0; i < N; i++) {
		sgpr_tie(g.kp[i]), sgpr_tie(g.kv[i]), sgpr_tie(g.ki[i]);
		if constexpr (VSAT) sgpr_tie(g.vsat[i]);
	}
}
// JointTask.cpp:299-345, S = I. use_vsat is batch-uniform: one branch around two loops, each fetching its gains in one burst.
template <class Rows>
DI void fast_jt_law(const JtGains& g, bool use_vsat, const RobotCtx& rc, const Rows& r, JtEarly& e) {
	if (use_vsat) {
		UNROLL for (int i = 0; i < N; i++) {
			const real qd = r.law_goal(i);
			e.ddq[i] = r.law_goal(2 * N + i);
			const real integ = fma(rc.q[i] - qd, g.dt, r.state(i));
			e.integ[i] = integ;
			const real kvi = gain_pinv(g.kv[i]);
			real dv = -g.kp[i] * kvi * (rc.q[i] - qd) - g.ki[i] * kvi * integ;
			dv = fmin(fmax(dv, -g.vsat[i]), g.vsat[i]);
			e.f[i] = -g.kv[i] * (rc.dq[i] - dv);
		}
	} else {
		UNROLL for (int i = 0; i < N; i++) {
			const real qd = r.law_goal(i), dqd = r.law_goal(N + i);
			e.ddq[i] = r.law_goal(2 * N + i);
			const real integ = fma(rc.q[i] - qd, g.dt, r.state(i));
			e.integ[i] = integ;
			e.f[i] = -g.kp[i] * (rc.q[i] - qd) - g.kv[i] * (rc.dq[i] - dqd) - g.ki[i] * integ;
		}
	}
}

// the same with the gains fetched here (the forms that evaluate the law ahead of the chain)
template <class Rows>
DI void fast_jt_early(const FastJt& t1, bool use_vsat, const RobotCtx& rc, const Rows& r, JtEarly& e) {
	JtGains g;
	if (use_vsat)
		jt_gains_burst<true>(t1, g);
	else
		jt_gains_burst<false>(t1, g);
	fast_jt_law(g, use_vsat, rc, r, e);
}

// Scheduling fence between phases (and a marker in the ISA for per-phase inspection): the kernel is
// one huge basic block, and without fences the scheduler interleaves phases and inflates the live set.
#define SAI2B_PHASE() do { __builtin_amdgcn_sched_barrier(0); asm volatile("; SAI2B_PHASE_MARK"); __builtin_amdgcn_sched_barrier(0); } while (0)
#if defined(__HIP_DEVICE_COMPILE__)
#define SAI2B_CHAIN_PHASE() SAI2B_PHASE()
#endif
}  // namespace sai2b
#include "sai2b_chain.h"
namespace sai2b {

// ---- Input staging of tick_fast_kernel (used by FAST = 2; FAST = 1 keeps its loads in registers). Every per-robot
// row the fast tick reads before its Cholesky part, besides q, goes global -> LDS by DMA (global_load_lds) at kernel
// entry, while the model phase runs from q alone, and is read back from LDS after one barrier. The LDS image is
// [row][64] doubles, one column per lane of the (single-wavefront) workgroup:
//   dq (N) | MotionForceTask law_goals (24) and state (6) | one pad row when the count is odd
//   | the MotionForceTask istate row IS_NTYPES (64 ints)
//   | FAST == 2 without payload: 35 rows the DMA never writes, the model phase's results parked by the lane itself
//     inside the window: M's lower triangle (28, row i (i + 1) / 2 + j) and g (7). M and g are then never live in
//     registers across the certificate or the control law; fast_tick reads M where it consumes it (LdsSym).
// 37 632 bytes for FAST = 2. The force-space rows (MotionForceTask goals 24-29, sensed, state 6-11) are not staged: they
// stay plain loads after the barrier (StagedRows). Nor are the JointTask's law_goals (3N) and state (N): its law is only
// ever needed as two dot products with the nullspace vector a, so it is evaluated behind a, from plain loads issued
// ahead of the whole factor chain, which hides them (JtLate). That is what makes room for M and g within
// 40 KiB (4 workgroups per CU).
// PAY: the payload form of the kernel. Its CRBA needs the robot's payload, which arrives by the DMA, so its model phase
// stays behind the barrier and nothing is parked: the image is dq | JointTask law_goals and state (FAST == 2) |
// MotionForceTask rows | the ten payload rows (sai2b_set_link_payload) | pad | istate: 39 168 bytes for FAST = 2.
template <int FAST, bool PAY = false>
struct StageLayout {
	static constexpr bool JT_STAGED = FAST == 2 && PAY, PARKED = FAST == 2 && !PAY;
	static constexpr int DQ = 0, JG = N, JS = JG + (JT_STAGED ? 3 * N : 0), MG = JS + (JT_STAGED ? N : 0);
	static constexpr int MS = MG + 24, PLD = MS + 6, ROWS = PLD + (PAY ? PAYLOAD_ROWS : 0);
	static constexpr int PAIRS = (ROWS + 1) / 2;  // a 16-byte glds moves two rows (lanes 0-31: row 2i, 32-63: 2i+1)
	static constexpr int IROW = 2 * PAIRS;		 // the istate row, 256 bytes
	static constexpr int IMAGE = IROW * 64 + 32;	 // doubles the DMA writes; the parked rows start here
	static constexpr int MROWS = N * (N + 1) / 2;
	static constexpr int DOUBLES = IMAGE + (PARKED ? (MROWS + N) * 64 : 0);
};

// first element of image row k in the batched arrays (the pad row repeats the last one)
// (P: the kernel's copy of the FastBlock's entry group, already in registers: no DMA instruction waits for a row base)
template <int FAST, bool PAY = false>
DI const real* stage_row(const FastEntry& P, int k) {
	using S = StageLayout<FAST, PAY>;
	const int B = P.B;
	if (k >= S::ROWS) k = S::ROWS - 1;
	if (k < S::JG) return P.dq + (size_t)(k - S::DQ) * B;
	if (k < S::JS) return P.law_goals1 + (size_t)(k - S::JG) * B;
	if (k < S::MG) return P.state1 + (size_t)(k - S::JS) * B;
	if (k < S::MS) return P.law_goals0 + (size_t)(k - S::MG) * B;
	if constexpr (PAY) {
		if (k >= S::PLD) return P.payload + (size_t)(k - S::PLD) * B;
	}
	return P.state0 + (size_t)(k - S::MS) * B;
}

DI void glds(const void* src, real* lds, int bytes) {
	typedef __attribute__((address_space(1))) void gvoid;
	typedef __attribute__((address_space(3))) void lvoid;
	if (bytes == 16)
		__builtin_amdgcn_global_load_lds((gvoid*)src, (lvoid*)lds, 16, 0, 0);
	else
		__builtin_amdgcn_global_load_lds((gvoid*)src, (lvoid*)lds, 4, 0, 0);
}

// Issue the DMA of the whole image for the 64 robots from b0 on; all 64 lanes take part, also those past B (the
// source columns of lanes past B are clamped into the batch, and the columns they fill are never read).
template <int FAST, bool PAY = false>
DI void stage_issue(const FastEntry& P, real* img, int b0) {
	using S = StageLayout<FAST, PAY>;
	const int B = P.B, lane = threadIdx.x;
	if ((B & 1) == 0) {	 // every row starts 16-byte aligned: lane l moves robots col, col + 1 of row 2i + l / 32
		const int col = min(b0 + 2 * (lane & 31), B - 2);
		const bool hi = lane >= 32;
		UNROLL for (int i = 0; i < S::PAIRS; i++)
			glds((hi ? stage_row<FAST, PAY>(P, 2 * i + 1) : stage_row<FAST, PAY>(P, 2 * i)) + col, img + 2 * i * 64, 16);
	} else {  // odd batch: 4-byte DMA, two per row; lane l moves dword l % 2 of robot col
		UNROLL for (int h = 0; h < 2; h++) {
			const int col = min(b0 + 32 * h + (lane >> 1), B - 1);
			UNROLL for (int k = 0; k < S::ROWS; k++)
				glds((const int*)(stage_row<FAST, PAY>(P, k) + col) + (lane & 1), img + k * 64 + 32 * h, 4);
		}
	}
	glds(P.istate0 + (size_t)IS_NTYPES * B + min(b0 + lane, B - 1), img + S::IROW * 64, 4);
}

// The rows of one task as the fast kernel reads them after the barrier: staged rows from the image (this lane's
// column), force-space rows from HBM.
struct StagedRows {
	const DevTask& t;
	int B, b;
	const real* lg;	 // image row of law_goals row 0, at this lane's column
	const real* st;	 // same for state
	int st_rows;	 // state rows in the image
	DI real law_goal(int k) const { return lg[k * 64]; }
	DI real goal(int k) const { return ld(t.goals, k, B, b); }
	DI real sensed(int k) const { return ld(t.sensed, k, B, b); }
	DI real state(int k) const { return k < st_rows ? st[k * 64] : ld(t.state, k, B, b); }
};

// ---- The functions of sai2b_device.hpp that read a DevTask, restated on the FastBlock's copies (sai2b_params.h) for the
// headline body: the same expressions in the same order. The originals stay as they are, so that every other kernel compiles
// to the code it had.
// frame_pose()
DI void frame_pose(const FastPose& t, const Frames& F, real* x, real* R) {
	real Rl[9], pl[3];
	UNROLL for (int k = 0; k < 9; k++) Rl[k] = F.R[N - 1][k];
	UNROLL for (int k = 0; k < 3; k++) pl[k] = F.p[N - 1][k];
	UNROLL for (int i = 0; i < N - 1; i++)
		if (t.link == i) {
			UNROLL for (int k = 0; k < 9; k++) Rl[k] = F.R[i][k];
			UNROLL for (int k = 0; k < 3; k++) pl[k] = F.p[i][k];
		}
	UNROLL for (int k = 0; k < 3; k++)
		x[k] = fma(Rl[3 * k], t.frame_pos[0], fma(Rl[3 * k + 1], t.frame_pos[1], fma(Rl[3 * k + 2], t.frame_pos[2], pl[k])));
	mm<3, 3, 3>(Rl, t.frame_rot, R);
}
// jacobian()
template <class MD>
DI void jacobian(const MD& md, const FastPose& t, const Frames& F, const real* x, real* J) {
	UNROLL for (int i = 0; i < N; i++) {
		real z[3] = {F.R[i][2], F.R[i][5], F.R[i][8]};
		real d[3] = {x[0] - F.p[i][0], x[1] - F.p[i][1], x[2] - F.p[i][2]}, v[3];
		cross3(z, d, v);
		const bool on = i <= t.link, pris = md.jtype[i] != 0;
		UNROLL for (int k = 0; k < 3; k++) {
			J[k * N + i] = on ? (pris ? z[k] : v[k]) : 0.0;
			J[(3 + k) * N + i] = (on && !pris) ? z[k] : 0.0;
		}
	}
}
// mft_load(), its batch-uniform branches from the flags word (FastEntry::flags)
template <class Rows>
DI void fast_mft_load(int flags, const Rows& r, MftIn& in) {
	UNROLL for (int k = 0; k < 3; k++) {
		in.g_pos[k] = r.law_goal(k);
		in.g_v[k] = r.law_goal(12 + k);
		in.g_w[k] = r.law_goal(15 + k);
		in.g_a[k] = r.law_goal(18 + k);
		in.g_al[k] = r.law_goal(21 + k);
		in.g_f[k] = in.g_m[k] = in.s_f[k] = in.s_m[k] = 0;
	}
	UNROLL for (int k = 0; k < 9; k++) in.g_rot[k] = r.law_goal(3 + k);
	UNROLL for (int k = 0; k < 6; k++) in.integ[k] = r.state(k);
	UNROLL for (int k = 6; k < 12; k++) in.integ[k] = 0;
	if (flags & FB_USES_FORCE) {
		UNROLL for (int k = 0; k < 3; k++) {
			in.g_f[k] = r.goal(24 + k);
			in.g_m[k] = r.goal(27 + k);
		}
		if (flags & (FB_CL_FORCE | FB_CL_MOMENT)) {
			UNROLL for (int k = 0; k < 3; k++) {
				in.s_f[k] = r.sensed(k);
				in.s_m[k] = r.sensed(3 + k);
			}
		}
	}
	if (flags & (FB_CL_FORCE | FB_CL_MOMENT)) {
		UNROLL for (int k = 6; k < 12; k++) in.integ[k] = r.state(k);
	}
}
// mft_store_integrators()
DI void fast_mft_store_integrators(int flags, real* state, int B, int b, const MftIn& in) {
	UNROLL for (int k = 0; k < 6; k++) st(state, k, B, b, in.integ[k]);
	if (flags & FB_CL_FORCE) {
		UNROLL for (int k = 6; k < 9; k++) st(state, k, B, b, in.integ[k]);
	}
	if (flags & FB_CL_MOMENT) {
		UNROLL for (int k = 9; k < 12; k++) st(state, k, B, b, in.integ[k]);
	}
}
// the plain_motion branch of mft_law_vw()
DI void fast_mft_law_plain(const FastLaw& t, const real* v, const real* w, const real* x, const real* R, MftIn& in, real* Fu, real* Ff) {
	real oe[3];
	orientation_error(in.g_rot, R, oe);
	UNROLL for (int k = 0; k < 3; k++) {
		const real ex = x[k] - in.g_pos[k];
		in.integ[k] = fma(ex, t.dt, in.integ[k]);
		in.integ[3 + k] = fma(oe[k], t.dt, in.integ[3 + k]);
		Fu[k] = in.g_a[k] - t.kp_pos[k] * ex - t.kv_pos[k] * (v[k] - in.g_v[k]) - t.ki_pos[k] * in.integ[k];
		Fu[3 + k] = in.g_al[k] - t.kp_ori[k] * oe[k] - t.kv_ori[k] * (w[k] - in.g_w[k]) - t.ki_ori[k] * in.integ[3 + k];
		Ff[k] = Ff[3 + k] = 0;
	}
}

// A symmetric N x N matrix parked in the LDS image (StageLayout::PARKED): row i (i + 1) / 2 + j of this lane's column
// holds element (i, j), j <= i. Indexed like the array it stands in for, lower triangle only.
struct LdsSym {
	const real* col;
	DI real operator[](int k) const {
		const int i = k / N, j = k % N;
		return col[(i * (i + 1) / 2 + j) * 64];
	}
};

// Where fast_tick gets the second-level JointTask law from. JtGiven: evaluated by the caller (fast_jt_early).
struct JtGiven {
	const JtEarly& e;
	DI void prefetch() {}
	DI void prefetch_q() {}
	DI void project(const real* a, real& af, real& aacc) {
		UNROLL for (int i = 0; i < N; i++) {
			af = fma(a[i], e.f[i], af);
			aacc = fma(a[i], e.ddq[i], aacc);
		}
	}
};
// JtLate: nothing of the law exists until the nullspace vector does. prefetch() issues the plain loads of its 4N rows,
// ahead of the chain; prefetch_q() those of q (an L2 hit: the wavefront loaded these rows at entry), behind the QR, so
// that q is not live across it; project() evaluates the same fast_jt_early from them (dq from the image), stores the
// advanced integrators (the caller is past worklist_append: this lane is committed to the fast path) and forms the two
// dot products.
// EARLY: where the law's gains are fetched, as one burst either way. true: with q, behind the QR, so that their round trip is
// over long before the nullspace vector exists (some 44 scalar registers held until then). false: at the top of project().
// Chosen per kernel from its ISA: the BAKED forms have the registers to hold them, in the others holding them costs lane spills
// (tests/test_fast_scalar_waits_isa.py counts both).
template <bool EARLY>
struct JtLate {
	const FastJt& t1;  // the law's gains, where they lie in the parameter block
	bool use_vsat;
	const real* law_goals;	// the JointTask's rows
	real* state;
	int B, b;
	const real* dq;	 // image row of dq[0], at this lane's column
	const real* qrows;
	real lg[3 * N], s[N], q[N];
	JtGains g;
	struct Rows {
		const real *lg, *s;
		DI real law_goal(int k) const { return lg[k]; }
		DI real state(int k) const { return s[k]; }
	};
	DI void prefetch() {
		UNROLL for (int k = 0; k < 3 * N; k++) lg[k] = ld(law_goals, k, B, b);
		UNROLL for (int i = 0; i < N; i++) s[i] = ld(state, i, B, b);
	}
	DI void prefetch_q() {
		UNROLL for (int i = 0; i < N; i++) q[i] = ld(qrows, i, B, b);
		// the gains with them: their one round trip is over long before the nullspace vector exists
		if constexpr (EARLY) gains();
	}
	DI void gains() {
		if (use_vsat)
			jt_gains_burst<true>(t1, g);
		else
			jt_gains_burst<false>(t1, g);
	}
	DI void project(const real* a, real& af, real& aacc) {
		// Nothing in the law depends on a, and arithmetic without a dependency is free to move up to the loads, taking
		// the wait for them along: a[0] is the last element the back substitution produces, so tie q to it.
		RobotCtx rc;
		UNROLL for (int i = 0; i < N; i++) {
			asm volatile("" : "+v"(q[i]) : "v"(a[0]));
			rc.q[i] = q[i];
			rc.dq[i] = dq[i * 64];
		}
		JtEarly e;
		asm volatile("; SAI2B_MARK jt_law_begin");
		if constexpr (!EARLY) gains();
		fast_jt_law(g, use_vsat, rc, Rows{lg, s}, e);
		asm volatile("; SAI2B_MARK jt_law_end");
		UNROLL for (int i = 0; i < N; i++) st(state, i, B, b, e.integ[i]);
		JtGiven{e}.project(a, af, aacc);
	}
};

// The Cholesky part of the one-level fast tick, [full MotionForceTask]. J and M are the Jacobian and mass matrix at
// rc.q, Fu/Ff the task forces of the MotionForceTask law. No nullspace is needed, so the operational-space matrix is
// factored as a Gram matrix: bounded-inertia side -> Y = L^-1 J^T -> (Lambda for FULL decoupling) -> torques.
template <class Mat>
DI void fast_tick_mft(const DevParams& P, const real* J, const Mat& M, const real* Fu, const real* Ff, real* tau) {
	const DevTask& t0 = P.task[0];

	const bool mft_bie = t0.decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES;
	const bool mft_full = t0.decoupling == SAI2B_FULL_DYNAMIC_DECOUPLING;
	const bool any_bie = mft_bie;
	const real thr = t0.bie_threshold;
	// Phase A: bounded-inertia side (LB, YB = LB^-1 J^T, AB = YB^T YB, z = AB^-1 F_unit); YB dies here
	real LB[N * N], dB[N], z[6];
	UNROLL for (int i = 0; i < 6; i++) z[i] = Fu[i];
	if (any_bie) {
		real MB[N * N];
		UNROLL for (int i = 0; i < N; i++) UNROLL for (int j = 0; j <= i; j++) MB[i * N + j] = M[i * N + j];
		UNROLL for (int i = 0; i < N; i++) MB[i * N + i] = fmax(MB[i * N + i], thr);
		chol<N>(MB, LB, dB);
	}
	if (mft_bie) {	// Lambda_mod = (J Mb^-1 J^T)^-1
		real YB[N * 6], AB[36], LAB[36], dAB[6];
		UNROLL for (int c = 0; c < 6; c++) {
			real colb[N];
			UNROLL for (int i = 0; i < N; i++) colb[i] = J[c * N + i];
			solve_lower<N>(LB, dB, colb);
			UNROLL for (int i = 0; i < N; i++) YB[i * 6 + c] = colb[i];
		}
		UNROLL for (int i = 0; i < 6; i++) UNROLL for (int j = 0; j <= i; j++) {
			real s = 0;
			UNROLL for (int l = 0; l < N; l++) s = fma(YB[l * 6 + i], YB[l * 6 + j], s);
			AB[i * 6 + j] = s;
			AB[j * 6 + i] = s;
		}
		chol<6>(AB, LAB, dAB);
		solve_lower<6>(LAB, dAB, z);
		solve_lower_t<6>(LAB, dAB, z);
	}
	SAI2B_PHASE();
	// Phase B: M = L L^T, Y = L^-1 J^T; from here J and M are dead: tau_mft = J^T z = L (Y z)
	real L[N * N], dL[N], Y[N * 6];
	chol<N>(M, L, dL);
	UNROLL for (int c = 0; c < 6; c++) {
		real col[N];
		UNROLL for (int i = 0; i < N; i++) col[i] = J[c * N + i];
		solve_lower<N>(L, dL, col);
		UNROLL for (int i = 0; i < N; i++) Y[i * 6 + c] = col[i];
	}
	SAI2B_PHASE();
	// ---- A = J M^-1 J^T = Y^T Y and its factor: Lambda for FULL decoupling
	if (mft_full) {
		real A[36], LA[36], dA[6];
		UNROLL for (int i = 0; i < 6; i++) UNROLL for (int j = 0; j <= i; j++) {
			real s = 0;
			UNROLL for (int l = 0; l < N; l++) s = fma(Y[l * 6 + i], Y[l * 6 + j], s);
			A[i * 6 + j] = s;
			A[j * 6 + i] = s;
		}
		chol<6>(A, LA, dA);
		solve_lower<6>(LA, dA, z);	// Lambda_mod = Lambda = A^-1
		solve_lower_t<6>(LA, dA, z);
	}
	SAI2B_PHASE();
	// ---- MotionForceTask torques J^T (Lambda_mod F_unit + F_force) = L (Y z)   (SingularityHandler.cpp:307-309)
	UNROLL for (int i = 0; i < 6; i++) z[i] += Ff[i];
	real yz[N], tau_mft[N];
	mv<N, 6>(Y, z, yz);
	UNROLL for (int i = 0; i < N; i++) {
		real s = 0;
		UNROLL for (int k = 0; k <= i; k++) s = fma(L[i * N + k], yz[k], s);
		tau_mft[i] = s;
	}
	// (the copy stays: with it the one-level kernels compile to the instructions they had, profiles/one_chain_isa.txt)
	UNROLL for (int i = 0; i < N; i++) tau[i] = tau_mft[i];
}

// The two-level fast tick, [full MotionForceTask, full JointTask]: chain::tick2 (sai2b_chain.h) on this lane's J and M
// (M an array or LdsSym: it is read for the chain's factor, for M nv, and for the other factor where one is needed).
// One whitened chain Lx, Yx = Lx^-1 J^T on Mb (bounded-inertia MotionForceTask) or on M; Householder QR of Yx gives
// the factor R of J Mx^-1 J^T for the MotionForceTask solves and the nullspace direction w = Q e_6 in one pass; the
// projector is N = a bb^T with a, bb from nv = Lx^-T w and M nv. jt is the JointTask law (JtGiven or JtLate): its loads
// are issued ahead of the whole chain, which is what hides them.
// flags: FastEntry::flags, the tasks' decouplings among them; one bounded inertia estimate for the tasks that ask for it (the
// host checks that the thresholds agree, and FastChain holds the one that counts)
template <class Mat, class JT>
DI void fast_tick2(int flags, const FastChain& c, const real* J, const Mat& M, const real* Fu, const real* Ff, bool with_comp, JT& jt,
				   real* tau) {
	chain::tick2<N>(J, M, Fu, Ff, (flags & FB_MFT_BIE) != 0, (flags & FB_MFT_FULL) != 0, (flags & FB_JT_FULL) != 0,
					(flags & FB_JT_IMP) != 0, c.bie_threshold, with_comp, jt, tau);
}
template <bool HAS_JT, class Mat, class JT>
DI void fast_tick(const DevParams& P, const real* J, const Mat& M, const real* Fu, const real* Ff, int B, int b,
				  bool with_comp, JT& jt, real* tau) {
	if constexpr (!HAS_JT) {
		fast_tick_mft(P, J, M, Fu, Ff, tau);
	} else {
		fast_tick2(P.fast.entry.flags, P.fast.chain, J, M, Fu, Ff, with_comp, jt, tau);
	}
}

}  // namespace sai2b

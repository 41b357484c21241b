// sai2b_ik_law.h — damped least-squares inverse kinematics of one robot (include/sai2b.h "inverse kinematics"): a goal pose and
// a seed q in, a joint vector, five status values and a flags byte out. A pure function of the batch-uniform block, the robot's
// rows and its index, so ik_kernel (sai2b_ik.hip) and a CPU program (tests/cpp/ik_driver.cpp) run the same code. No HIP in here
// when a host compiler reads it.
// Every buffer is [row][stride]: the kernel passes its column (base + b) with stride B, the CPU program a robot of its own with
// stride 1. The chain is walked in the convention of include/sai2b_detfk.h (p += R xyz_i, R = R E_i, then the joint about / along
// z), in plain FP64.
// Written for one lane per robot: every array is indexed by loop counters that are compile-time constants once the loops are
// unrolled (the device build unrolls all of them but the solve's own loop). What is batch-uniform but not known at compile time
// (the task's link, the axes) is a wave-uniform test or a factor; what differs per lane is a select, never an index.
//
// ONE LOOP. A trip of the loop proposes a candidate q' (the start's seed, or q + d of a Levenberg-Marquardt step), evaluates the
// pose alone at q', accepts or rejects it, and builds the joint axes (the Jacobian) only for an accepted q'. A start is a
// candidate that is always accepted, so the forward kinematics stands in the code once per form. The loop is left when no lane
// of the wavefront has work left (SAI2B_IK_ANY: __any on the device, the lane's own flag on the CPU); a lane that is done waits
// with its execution bit off.
#pragma once
#include <cmath>
#include <cstddef>

#include "sai2b_reset_draw.h"

#if defined(__HIPCC__)
#define SAI2B_IK_HD __host__ __device__
#else
#define SAI2B_IK_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SAI2B_IK_UNROLL _Pragma("unroll")
#define SAI2B_IK_ANY(x) __any(x)
#else
#define SAI2B_IK_UNROLL
#define SAI2B_IK_ANY(x) (x)
#endif

namespace sai2b {

enum { IK_STREAM = 11 };  // streams 0-10 are the hardware's, the episode sampler's, the environment sampler's and the joint sensor's
enum { IK_FLAG_CONVERGED = 1, IK_FLAG_EXHAUSTED = 2, IK_FLAG_AT_LIMIT = 4, IK_FLAG_NONFINITE = 8 };
constexpr int IK_POSE_ROWS = 12;   // goal position 3, goal rotation 9 row-major
constexpr int IK_STATUS_ROWS = 5;  // |e_pos|, |e_rot| at q_out, iterations, start index, final mu
constexpr int IK_COUNTS = 4;	   // selected, converged, exhausted, non-finite
constexpr int IK_MAX_ITERATIONS = 200, IK_MAX_RESTARTS = 16;

// the batch-uniform part: the chain, the frame that is solved for, the clamped limits and the numbers of the law
template <int DOF>
struct IkLaw {
	double E[DOF][9], xyz[DOF][3];	// joint frame in the parent link
	int jtype[DOF];					// 0 revolute about, 1 prismatic along the joint frame's z
	double lo[DOF], hi[DOF];		// q_lower + margin, q_upper - margin; -inf, +inf without use_limits
	int link;						// the task's link
	double frame_pos[3], frame_rot[9];	// its control frame in that link
	double w2[6];					// the squares of W's diagonal: axes . (1, 1, 1, L^2, L^2, L^2)
	double sel[6];					// axes as 0 / 1, for the unweighted norms
	int max_iterations, restarts, use_limits;
	double tol_pos, tol_rot, mu0, mu_min, mu_max, mu_down, mu_up, step_max, rest_weight;
	unsigned key0, key1, first_robot, draw_id;
};

SAI2B_IK_HD inline bool ik_finite(double v) { return v - v == 0.0; }

// Forward kinematics of the control frame with given sines and cosines: x [3], R [9] row-major. JAC: also z_m (the world z of
// joint m's frame) and o_m (its world origin) of every joint, from which a Jacobian column is z_m x (x - o_m) ; z_m about a
// revolute joint and z_m ; 0 along a prismatic one.
template <int DOF, bool JAC>
SAI2B_IK_HD inline void ik_fk(const IkLaw<DOF>& G, const double (&q)[DOF], const double (&sn)[DOF], const double (&cs)[DOF], double x[3], double Rc[9],
							  double (&z)[DOF][3], double (&o)[DOF][3]) {
	double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
	SAI2B_IK_UNROLL
	for (int a = 0; a < 3; a++) x[a] = 0.0;
	SAI2B_IK_UNROLL
	for (int a = 0; a < 9; a++) Rc[a] = 0.0;
	SAI2B_IK_UNROLL
	for (int i = 0; i < DOF; i++) {
		if (i <= G.link) {	// wave-uniform: the joints beyond the task's link move nothing
			double RE[9];
			SAI2B_IK_UNROLL
			for (int r = 0; r < 3; r++) {
				p[r] = p[r] + (R[3 * r] * G.xyz[i][0] + R[3 * r + 1] * G.xyz[i][1] + R[3 * r + 2] * G.xyz[i][2]);
				SAI2B_IK_UNROLL
				for (int c = 0; c < 3; c++) RE[3 * r + c] = R[3 * r] * G.E[i][c] + R[3 * r + 1] * G.E[i][3 + c] + R[3 * r + 2] * G.E[i][6 + c];
			}
			if (G.jtype[i]) {
				SAI2B_IK_UNROLL
				for (int r = 0; r < 3; r++) {
					p[r] = p[r] + RE[3 * r + 2] * q[i];
					R[3 * r] = RE[3 * r], R[3 * r + 1] = RE[3 * r + 1], R[3 * r + 2] = RE[3 * r + 2];
				}
			} else {
				SAI2B_IK_UNROLL
				for (int r = 0; r < 3; r++) {
					R[3 * r] = cs[i] * RE[3 * r] + sn[i] * RE[3 * r + 1];
					R[3 * r + 1] = cs[i] * RE[3 * r + 1] - sn[i] * RE[3 * r];
					R[3 * r + 2] = RE[3 * r + 2];
				}
			}
			if (JAC) {
				SAI2B_IK_UNROLL
				for (int r = 0; r < 3; r++) z[i][r] = R[3 * r + 2], o[i][r] = p[r];
			}
			if (G.link == i) {	// wave-uniform: the control frame behind this link's frame
				SAI2B_IK_UNROLL
				for (int r = 0; r < 3; r++) {
					x[r] = p[r] + (R[3 * r] * G.frame_pos[0] + R[3 * r + 1] * G.frame_pos[1] + R[3 * r + 2] * G.frame_pos[2]);
					SAI2B_IK_UNROLL
					for (int c = 0; c < 3; c++)
						Rc[3 * r + c] = R[3 * r] * G.frame_rot[c] + R[3 * r + 1] * G.frame_rot[3 + c] + R[3 * r + 2] * G.frame_rot[6 + c];
				}
			}
		}
	}
}

// r = the rotation vector of D = Rg R^T in the world frame, the full logarithm. With c = (tr D - 1) / 2 clamped to [-1, 1],
// v = vee(D - D^T) / 2 (= sin(theta) axis), s = |v| and theta = atan2(s, c):
//   c >= 0 (theta <= pi / 2):  r = (theta / s) v, and r = v when s < 1e-12 (near 0: the factor is 1 to 2e-25)
//   c <  0 (theta >  pi / 2):  the axis from the symmetric part, M = (D + D^T) / 2 - c I = (1 - c) a a^T: with k the first largest
//                              diagonal entry of M, a = M[:, k] / sqrt((1 - c) M[k][k]), negated when a . v < 0; r = theta a. Near pi
//                              this keeps its accuracy where v vanishes; at pi exactly the sign of a is that of its component k.
// Both forms agree where they meet, so the branch hangs on no rounding.
SAI2B_IK_HD inline void ik_rotation_log(const double Rg[9], const double R[9], double r[3]) {
	double D[9];
	SAI2B_IK_UNROLL
	for (int i = 0; i < 3; i++) {
		SAI2B_IK_UNROLL
		for (int j = 0; j < 3; j++) D[3 * i + j] = Rg[3 * i] * R[3 * j] + Rg[3 * i + 1] * R[3 * j + 1] + Rg[3 * i + 2] * R[3 * j + 2];
	}
	double c = 0.5 * ((D[0] + D[4] + D[8]) - 1.0);
	c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
	const double v[3] = {0.5 * (D[7] - D[5]), 0.5 * (D[2] - D[6]), 0.5 * (D[3] - D[1])};
	const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	const double theta = atan2(s, c);
	if (c >= 0.0) {
		const double f = s < 1e-12 ? 1.0 : theta / s;
		SAI2B_IK_UNROLL
		for (int a = 0; a < 3; a++) r[a] = f * v[a];
	} else {
		const double m0 = D[0] - c, m1 = D[4] - c, m2 = D[8] - c;
		const double s01 = 0.5 * (D[1] + D[3]), s02 = 0.5 * (D[2] + D[6]), s12 = 0.5 * (D[5] + D[7]);
		const bool k1 = m1 > m0 && m1 >= m2, k2 = m2 > m0 && m2 > m1;  // else k = 0
		const double col0 = k2 ? s02 : (k1 ? s01 : m0), col1 = k2 ? s12 : (k1 ? m1 : s01), col2 = k2 ? m2 : (k1 ? s12 : s02);
		const double mk = k2 ? m2 : (k1 ? m1 : m0);
		const double inv = 1.0 / sqrt((1.0 - c) * mk);
		double a0 = col0 * inv, a1 = col1 * inv, a2 = col2 * inv;
		const double sign = (a0 * v[0] + a1 * v[1] + a2 * v[2]) < 0.0 ? -theta : theta;
		r[0] = sign * a0, r[1] = sign * a1, r[2] = sign * a2;
	}
}

// the seed of start n >= 1: uniform in the clamped limits (finite: the validator's condition on restarts > 0), joint i from word
// i mod 4 of call i / 4 of stream IK_STREAM, counter (n, draw_id, 256 stream + call, first_robot + robot)
template <int DOF>
SAI2B_IK_HD inline void ik_restart_seed(const IkLaw<DOF>& G, unsigned n, unsigned robot, double (&q)[DOF]) {
	SAI2B_IK_UNROLL
	for (int c = 0; c < (DOF + 3) / 4; c++) {
		double u[4];
		rs_uniforms4(n, G.draw_id, IK_STREAM, (unsigned)c, G.first_robot + robot, G.key0, G.key1, u);
		SAI2B_IK_UNROLL
		for (int j = 0; j < 4; j++)
			if (4 * c + j < DOF) q[4 * c + j] = rs_lerp(G.lo[4 * c + j], G.hi[4 * c + j], u[j]);
	}
}

// One robot. live: the robot is selected (a lane that is not takes part in the wave-uniform loop exit and touches no memory).
// goal: its pose rows (position 3, rotation 9 row-major); rest: its rest posture rows or NULL (rest_weight == 0); seed: its seed q;
// robot: its index in its context (the draws add first_robot). q_out [DOF] and status [IK_STATUS_ROWS]: its columns, written
// unless the robot is not finite. Returns the flags byte (0 for a lane that is not live).
template <int DOF>
SAI2B_IK_HD inline int ik_law(const IkLaw<DOF>& G, bool live, const double* goal, const double* rest, const double* seed, size_t sB, unsigned robot,
							  double* q_out, double* status) {
	double xg[3], Rg[9], q[DOF], qr[DOF];
	bool finite = true;
	SAI2B_IK_UNROLL
	for (int a = 0; a < 3; a++) xg[a] = 0.0;
	SAI2B_IK_UNROLL
	for (int a = 0; a < 9; a++) Rg[a] = 0.0;
	SAI2B_IK_UNROLL
	for (int i = 0; i < DOF; i++) q[i] = 0.0, qr[i] = 0.0;
	if (live) {
		SAI2B_IK_UNROLL
		for (int a = 0; a < 3; a++) xg[a] = goal[(size_t)a * sB], finite = finite && ik_finite(xg[a]);
		SAI2B_IK_UNROLL
		for (int a = 0; a < 9; a++) Rg[a] = goal[(size_t)(3 + a) * sB], finite = finite && ik_finite(Rg[a]);
		SAI2B_IK_UNROLL
		for (int i = 0; i < DOF; i++) q[i] = seed[(size_t)i * sB], finite = finite && ik_finite(q[i]);
		if (rest) {
			SAI2B_IK_UNROLL
			for (int i = 0; i < DOF; i++) qr[i] = rest[(size_t)i * sB], finite = finite && ik_finite(qr[i]);
		}
	}
	const double nu = rest ? G.rest_weight : 0.0;
	// the state of the solve
	double z[DOF][3], o[DOF][3], x[3], e[6], E2 = HUGE_VAL, mu = G.mu0;
	double qb[DOF], best_E2 = HUGE_VAL, best_pos = HUGE_VAL, best_rot = HUGE_VAL;
	int start = 0, best_start = 0, k = 0, it = 0;
	bool fresh = true, converged = false, active = live && finite;
	SAI2B_IK_UNROLL
	for (int i = 0; i < DOF; i++) {
		qb[i] = 0.0;
		SAI2B_IK_UNROLL
		for (int a = 0; a < 3; a++) z[i][a] = 0.0, o[i][a] = 0.0;
	}
	SAI2B_IK_UNROLL
	for (int a = 0; a < 3; a++) x[a] = 0.0;
	SAI2B_IK_UNROLL
	for (int a = 0; a < 6; a++) e[a] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
	for (;;) {
		if (!SAI2B_IK_ANY(active)) break;
		if (active) {
			// ---- the candidate
			double qn[DOF];
			if (fresh) {
				if (start > 0) ik_restart_seed<DOF>(G, (unsigned)start, robot, q);
				SAI2B_IK_UNROLL
				for (int i = 0; i < DOF; i++) qn[i] = q[i];
			} else {
				// (J^T W^2 J + (mu + nu) I) d = J^T W^2 e + nu (q_rest - q): the lower triangle, Cholesky, two substitutions
				double H[DOF][DOF], d[DOF];
				SAI2B_IK_UNROLL
				for (int i = 0; i < DOF; i++) {
					d[i] = nu * (qr[i] - q[i]);
					SAI2B_IK_UNROLL
					for (int j = 0; j <= i; j++) H[i][j] = i == j ? mu + nu : 0.0;
				}
				SAI2B_IK_UNROLL
				for (int r = 0; r < 6; r++) {
					if (G.w2[r] != 0.0) {  // wave-uniform
						double Jr[DOF];
						SAI2B_IK_UNROLL
						for (int m = 0; m < DOF; m++) {
							double v;
							if (r < 3) {
								const int a = (r + 1) % 3, b = (r + 2) % 3;
								v = G.jtype[m] ? z[m][r] : z[m][a] * (x[b] - o[m][b]) - z[m][b] * (x[a] - o[m][a]);
							} else {
								v = G.jtype[m] ? 0.0 : z[m][r - 3];
							}
							Jr[m] = m <= G.link ? v : 0.0;
						}
						const double we = G.w2[r] * e[r];
						SAI2B_IK_UNROLL
						for (int i = 0; i < DOF; i++) {
							d[i] += Jr[i] * we;
							const double wj = G.w2[r] * Jr[i];
							SAI2B_IK_UNROLL
							for (int j = 0; j <= i; j++) H[i][j] += wj * Jr[j];
						}
					}
				}
				SAI2B_IK_UNROLL
				for (int j = 0; j < DOF; j++) {
					SAI2B_IK_UNROLL
					for (int l = 0; l < j; l++) H[j][j] -= H[j][l] * H[j][l];
					H[j][j] = sqrt(H[j][j]);
					const double inv = 1.0 / H[j][j];
					SAI2B_IK_UNROLL
					for (int i = j + 1; i < DOF; i++) {
						SAI2B_IK_UNROLL
						for (int l = 0; l < j; l++) H[i][j] -= H[i][l] * H[j][l];
						H[i][j] *= inv;
					}
				}
				SAI2B_IK_UNROLL
				for (int i = 0; i < DOF; i++) {
					SAI2B_IK_UNROLL
					for (int l = 0; l < i; l++) d[i] -= H[i][l] * d[l];
					d[i] /= H[i][i];
				}
				SAI2B_IK_UNROLL
				for (int i = DOF - 1; i >= 0; i--) {
					SAI2B_IK_UNROLL
					for (int l = i + 1; l < DOF; l++) d[i] -= H[l][i] * d[l];
					d[i] /= H[i][i];
				}
				double big = 0.0;
				SAI2B_IK_UNROLL
				for (int i = 0; i < DOF; i++) big = fabs(d[i]) > big ? fabs(d[i]) : big;
				const double scale = big > G.step_max ? G.step_max / big : 1.0;
				SAI2B_IK_UNROLL
				for (int i = 0; i < DOF; i++) qn[i] = q[i] + scale * d[i];
			}
			SAI2B_IK_UNROLL
			for (int i = 0; i < DOF; i++) {
				qn[i] = qn[i] < G.lo[i] ? G.lo[i] : qn[i];
				qn[i] = qn[i] > G.hi[i] ? G.hi[i] : qn[i];
			}
			// ---- the pose alone at the candidate
			double sn[DOF], cs[DOF], xn[3], Rn[9], en[6];
			SAI2B_IK_UNROLL
			for (int i = 0; i < DOF; i++) sn[i] = sin(qn[i]), cs[i] = cos(qn[i]);
			ik_fk<DOF, false>(G, qn, sn, cs, xn, Rn, z, o);
			SAI2B_IK_UNROLL
			for (int a = 0; a < 3; a++) en[a] = xg[a] - xn[a];
			ik_rotation_log(Rg, Rn, en + 3);
			double En = 0.0;
			SAI2B_IK_UNROLL
			for (int a = 0; a < 6; a++) En += G.w2[a] * (en[a] * en[a]);
			// ---- accept or reject
			const bool accept = fresh || En < E2;  // false for a NaN
			if (accept) {
				SAI2B_IK_UNROLL
				for (int i = 0; i < DOF; i++) q[i] = qn[i];
				SAI2B_IK_UNROLL
				for (int a = 0; a < 6; a++) e[a] = en[a];
				E2 = En;
				ik_fk<DOF, true>(G, qn, sn, cs, x, Rn, z, o);  // the joint axes of the accepted iterate
			}
			if (fresh) {
				mu = G.mu0;
			} else {
				const double down = mu * G.mu_down, up = mu * G.mu_up;
				mu = accept ? (down > G.mu_min ? down : G.mu_min) : (up < G.mu_max ? up : G.mu_max);
				k++, it++;
			}
			fresh = false;
			// ---- converged, or this start is spent
			const double ep = sqrt(G.sel[0] * (e[0] * e[0]) + G.sel[1] * (e[1] * e[1]) + G.sel[2] * (e[2] * e[2]));
			const double er = sqrt(G.sel[3] * (e[3] * e[3]) + G.sel[4] * (e[4] * e[4]) + G.sel[5] * (e[5] * e[5]));
			converged = ep <= G.tol_pos && er <= G.tol_rot;
			if (converged || k >= G.max_iterations) {
				if (converged || start == 0 || E2 < best_E2) {
					SAI2B_IK_UNROLL
					for (int i = 0; i < DOF; i++) qb[i] = q[i];
					best_E2 = E2, best_pos = ep, best_rot = er, best_start = start;
				}
				if (converged || start >= G.restarts) {
					active = false;
				} else {
					start++, k = 0, fresh = true;
				}
			}
		}
	}
	if (!live) return 0;
	if (!finite) return IK_FLAG_NONFINITE;
	int flags = converged ? IK_FLAG_CONVERGED : IK_FLAG_EXHAUSTED;
	SAI2B_IK_UNROLL
	for (int i = 0; i < DOF; i++) {
		q_out[(size_t)i * sB] = qb[i];
		if (G.use_limits && (qb[i] <= G.lo[i] || qb[i] >= G.hi[i])) flags |= IK_FLAG_AT_LIMIT;
	}
	status[0] = best_pos, status[sB] = best_rot, status[2 * sB] = (double)it, status[3 * sB] = (double)best_start, status[4 * sB] = mu;
	return flags;
}

}  // namespace sai2b

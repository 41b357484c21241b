// sai2b_sim.hip — simulation harness: rigid-body forward dynamics of the batch,
// state resident in HBM between control ticks.
//
// The reference's examples close the loop through the external sai2-simulation
// (examples/05-...cpp:215-236: setJointTorques / integrate / getJointPositions); nothing of it is in
// the reference tree, so the dynamics here are the textbook ones and the integrator is defined by
// this file: the joint torques are held over the control period dt, which is split into `substeps`
// semi-implicit Euler steps   dq += h M(q)^-1 (tau - b(q, dq)),   q += h dq,
// with b = C(q, dq) dq (+ g(q) when asked) from a recursive Newton-Euler pass in world coordinates.
// One lane per robot, as everywhere in this library; FK and the mass matrix are the tick kernel's own.
#include <hip/hip_runtime.h>

#include "sai2b_body_contact_law.h"
#include "sai2b_device.hpp"
#include "sai2b_fast.hpp"
#include "sai2b_launch.h"

namespace sai2b {

// b(q, dq) = C dq (+ g): Newton-Euler with zero joint accelerations. World-frame angular velocity w,
// angular acceleration al, linear acceleration a of each joint-frame origin; forces F and moments Nn
// about the link COMs; backward accumulation to the joint axes.
// pl: the plant's payload, a second body on link pl.link (Payload with link < 0: none; NoPayload: the code without it)
template <class MD, class PL>
DI void bias_forces(const MD& md, const Frames& Fr, const real* dq, bool with_gravity, real* b, const PL& pl) {
	real F[N][3], Nn[N][3], rc[N][3];
	[[maybe_unused]] real Fp[3] = {0, 0, 0}, Np[3] = {0, 0, 0}, rp[3] = {0, 0, 0};  // the payload's force, moment about its COM, COM from the link origin
	real w[3] = {0, 0, 0}, al[3] = {0, 0, 0}, a[3] = {0, 0, 0}, o[3] = {0, 0, 0};
	if (with_gravity) {
		UNROLL for (int k = 0; k < 3; k++) a[k] = -md.gravity[k];
	}
	UNROLL for (int i = 0; i < N; i++) {
		const real* R = Fr.R[i];
		const real z[3] = {R[2], R[5], R[8]};
		real r[3], t1[3], t2[3], t3[3];
		UNROLL for (int k = 0; k < 3; k++) r[k] = Fr.p[i][k] - o[k];
		cross3(al, r, t1);
		cross3(w, r, t2);
		cross3(w, t2, t3);
		UNROLL for (int k = 0; k < 3; k++) a[k] += t1[k] + t3[k];
		real zq[3] = {z[0] * dq[i], z[1] * dq[i], z[2] * dq[i]};
		cross3(w, zq, t1);
		const bool pris = md.jtype[i] != 0;
		UNROLL for (int k = 0; k < 3; k++) {
			if (pris) {	 // sliding frame: Coriolis acceleration of its origin, no change of the angular motion
				a[k] += 2 * t1[k];
			} else {
				w[k] += zq[k];
				al[k] += t1[k];
			}
			o[k] = Fr.p[i][k];
		}
		UNROLL for (int k = 0; k < 3; k++)
			rc[i][k] = fma(R[3 * k], md.com[i][0], fma(R[3 * k + 1], md.com[i][1], R[3 * k + 2] * md.com[i][2]));
		real ac[3];
		cross3(al, rc[i], t1);
		cross3(w, rc[i], t2);
		cross3(w, t2, t3);
		UNROLL for (int k = 0; k < 3; k++) ac[k] = a[k] + t1[k] + t3[k];
		// I_world x = R I_link R^T x
		const real* li = md.inertia[i];
		real Il[9] = {li[0], li[3], li[4], li[3], li[1], li[5], li[4], li[5], li[2]};
		real u[3], Iu[3], Ial[3], Iw[3];
		mv_t<3, 3>(R, al, u);
		mv<3, 3>(Il, u, Iu);
		mv<3, 3>(R, Iu, Ial);
		mv_t<3, 3>(R, w, u);
		mv<3, 3>(Il, u, Iu);
		mv<3, 3>(R, Iu, Iw);
		cross3(w, Iw, t1);
		UNROLL for (int k = 0; k < 3; k++) {
			F[i][k] = md.mass[i] * ac[k];
			Nn[i][k] = Ial[k] + t1[k];
		}
		if constexpr (PL::on) if (pl.link == i) {
			UNROLL for (int k = 0; k < 3; k++) rp[k] = fma(R[3 * k], pl.c[0], fma(R[3 * k + 1], pl.c[1], R[3 * k + 2] * pl.c[2]));
			cross3(al, rp, t1);
			cross3(w, rp, t2);
			cross3(w, t2, t3);
			const real* pi = pl.I;
			real Ip[9] = {pi[0], pi[3], pi[4], pi[3], pi[1], pi[5], pi[4], pi[5], pi[2]};
			mv_t<3, 3>(R, al, u);
			mv<3, 3>(Ip, u, Iu);
			mv<3, 3>(R, Iu, Ial);
			mv_t<3, 3>(R, w, u);
			mv<3, 3>(Ip, u, Iu);
			mv<3, 3>(R, Iu, Iw);
			real t4[3];
			cross3(w, Iw, t4);
			UNROLL for (int k = 0; k < 3; k++) {
				Fp[k] = pl.m * (a[k] + t1[k] + t3[k]);
				Np[k] = Ial[k] + t4[k];
			}
		}
	}
	real f[3] = {0, 0, 0}, n[3] = {0, 0, 0};
	UNROLL for (int i = N - 1; i >= 0; i--) {
		real t1[3];
		cross3(rc[i], F[i], t1);
		if (i + 1 < N) {
			real d[3] = {Fr.p[i + 1][0] - Fr.p[i][0], Fr.p[i + 1][1] - Fr.p[i][1], Fr.p[i + 1][2] - Fr.p[i][2]}, t2[3];
			cross3(d, f, t2);
			UNROLL for (int k = 0; k < 3; k++) n[k] += t2[k];
		}
		UNROLL for (int k = 0; k < 3; k++) {
			n[k] += Nn[i][k] + t1[k];
			f[k] += F[i][k];
		}
		if constexpr (PL::on) if (pl.link == i) {
			cross3(rp, Fp, t1);
			UNROLL for (int k = 0; k < 3; k++) {
				n[k] += Np[k] + t1[k];
				f[k] += Fp[k];
			}
		}
		const real* pr = (md.jtype[i] != 0) ? f : n;  // prismatic: the force along the axis
		b[i] = Fr.R[i][2] * pr[0] + Fr.R[i][5] * pr[1] + Fr.R[i][8] * pr[2];
	}
}

// ---- contact of the plant (sai2b_set_contact): up to four points fixed to one link against one plane per robot.
// NoContact: sim_kernel compiles to what it is without the feature. The law (DESIGN "Contact in the simulated plant"):
//   delta = n . (p0 - x_k), vn = n . v_k, f_n = max(0, k max(0, delta) (1 - d vn)), v_t = v_k - vn n,
//   F_k = f_n n - mu f_n v_t / sqrt(|v_t|^2 + v_eps^2)      the force ON the robot, world frame
// continuous in the state everywhere (no jump at touch-down or lift-off, regularised Coulomb friction).
struct NoContact {
	static constexpr bool on = false;
};
struct Contact {
	static constexpr bool on = true;
	real p0[3], n[3], k, d, mu;	 // the robot's own plane: rows of the [9][B] buffer
};
constexpr int CONTACT_MAX_POINTS = SAI2B_MAX_CONTACT_POINTS;
// o: the origin of the step's coordinates (fk<true>: joint 0's frame origin); the plane point is taken relative to it
DI void contact_load(const real* rows, const double* o, int B, int b, Contact& ct) {
	UNROLL for (int k = 0; k < 3; k++) {
		ct.p0[k] = ld(rows, k, B, b) - o[k];
		ct.n[k] = ld(rows, 3 + k, B, b);
	}
	ct.k = ld(rows, 6, B, b);
	ct.d = ld(rows, 7, B, b);
	ct.mu = ld(rows, 8, B, b);
}
// frame of a batch-uniform link without dynamic register indexing (as frame_pose)
DI void link_frame(int link, const Frames& F, real* R, real* p) {
	UNROLL for (int k = 0; k < 9; k++) R[k] = F.R[N - 1][k];
	UNROLL for (int k = 0; k < 3; k++) p[k] = F.p[N - 1][k];
	UNROLL for (int i = 0; i < N - 1; i++)
		if (link == i) {
			UNROLL for (int k = 0; k < 9; k++) R[k] = F.R[i][k];
			UNROLL for (int k = 0; k < 3; k++) p[k] = F.p[i][k];
		}
}
// One point: world position x, force Fk on the robot, penetration and normal force. The point's velocity comes from the
// joints at or below the link, J_k is never formed: a revolute joint contributes dq_i z_i x (x - p_i), a prismatic one dq_i z_i.
template <class MD>
DI void contact_point(const MD& md, const DevParams& P, const Contact& ct, const Frames& Fr, const real* Rl, const real* pl, int k,
					  const real* dq, real* x, real* Fk, real& delta, real& fn) {
	const double* c = P.contact_points[k];
	UNROLL for (int a = 0; a < 3; a++) x[a] = fma(Rl[3 * a], c[0], fma(Rl[3 * a + 1], c[1], fma(Rl[3 * a + 2], c[2], pl[a])));
	real v[3] = {0, 0, 0};
	UNROLL for (int i = 0; i < N; i++) {
		const real z[3] = {Fr.R[i][2], Fr.R[i][5], Fr.R[i][8]};
		const real r[3] = {x[0] - Fr.p[i][0], x[1] - Fr.p[i][1], x[2] - Fr.p[i][2]};
		real zr[3];
		cross3(z, r, zr);
		const bool pris = md.jtype[i] != 0;
		const real w = i <= P.contact_link ? dq[i] : 0.0;
		UNROLL for (int a = 0; a < 3; a++) v[a] = fma(w, pris ? z[a] : zr[a], v[a]);
	}
	const real* n = ct.n;
	delta = n[0] * (ct.p0[0] - x[0]) + n[1] * (ct.p0[1] - x[1]) + n[2] * (ct.p0[2] - x[2]);
	const real vn = n[0] * v[0] + n[1] * v[1] + n[2] * v[2];
	fn = fmax(0.0, ct.k * fmax(0.0, delta) * (1.0 - ct.d * vn));
	real vt[3];
	UNROLL for (int a = 0; a < 3; a++) vt[a] = v[a] - vn * n[a];
	const real s = ct.mu * fn / sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2] + P.contact_v_eps * P.contact_v_eps);
	UNROLL for (int a = 0; a < 3; a++) Fk[a] = fn * n[a] - s * vt[a];
}
// tc = sum_k J_k^T F_k: row i gets z_i . ((x_k - p_i) x F_k) from a revolute joint, z_i . F_k from a prismatic one
template <class MD>
DI void contact_torques(const MD& md, const DevParams& P, const Contact& ct, const Frames& Fr, const real* dq, real* tc) {
	real Rl[9], pl[3];
	link_frame(P.contact_link, Fr, Rl, pl);
	UNROLL for (int i = 0; i < N; i++) tc[i] = 0;
	UNROLL for (int k = 0; k < CONTACT_MAX_POINTS; k++) {
		if (k < P.contact_n_points) {  // batch-uniform
			real x[3], Fk[3], delta, fn;
			contact_point(md, P, ct, Fr, Rl, pl, k, dq, x, Fk, delta, fn);
			UNROLL for (int i = 0; i < N; i++) {
				const real z[3] = {Fr.R[i][2], Fr.R[i][5], Fr.R[i][8]};
				const real r[3] = {x[0] - Fr.p[i][0], x[1] - Fr.p[i][1], x[2] - Fr.p[i][2]};
				real m[3];
				cross3(r, Fk, m);
				const real* pr = (md.jtype[i] != 0) ? Fk : m;
				const real t = z[0] * pr[0] + z[1] * pr[1] + z[2] * pr[2];
				tc[i] += i <= P.contact_link ? t : 0.0;
			}
		}
	}
}
// A second wrench ON the robot for the same ideal sensor (the external wrench of sai2b_set_external_wrench): F, M about x, world
// frame. NoReading: contact_report compiles to what it is without one. add (batch-uniform): the sensor task is the contact's
// own, the sum of the two readings is stored once.
struct NoReading {
	static constexpr bool on = false;
};
struct WrenchReading {
	static constexpr bool on = true;
	bool add;
	real x[3], F[3], M[3];
};
// the reading of the ideal sensor of task t from the wrench ON the robot, Ft and Mt about the control point x_c (Rc: the
// control frame): f_s = R_s^T (-Ft), m_s = R_s^T (-(Mt - (o_s - x_c) x Ft)), stored into the task's sensed rows. For the
// external wrench's own sensor; contact_report holds the same statements in line (behind a call its kernels compile differently)
DI void sensor_store(const DevTask& t, const real* Rc, const real* Ft, const real* Mt, int B, int b) {
	real Rs[9], os[3], ms_w[3], t1[3], fs[3], ms[3];
	mm<3, 3, 3>(Rc, t.sensor_rot, Rs);
	mv3(Rc, t.sensor_pos, os);	// o_s - x_c
	cross3(os, Ft, t1);
	// -sum (x_k - o_s) x F_k = -(sum (x_k - x_c) x F_k - (o_s - x_c) x sum F_k)
	UNROLL for (int a = 0; a < 3; a++) {
		ms_w[a] = t1[a] - Mt[a];
		t1[a] = -Ft[a];
	}
	mv_t<3, 3>(Rs, t1, fs);
	mv_t<3, 3>(Rs, ms_w, ms);
	UNROLL for (int a = 0; a < 3; a++) {
		st(t.sensed, a, B, b, fs[a]);
		st(t.sensed, 3 + a, B, b, ms[a]);
	}
}
// After the last substep: the status rows [2 * 4 + 6][B] (per point delta and f_n, then sum F_k and sum (x_k - x_c) x F_k in
// the world frame; x_c: the control point of the sensor task, the contact link's origin without one), the count of robots
// in contact, and the reading of the ideal force / moment sensor: the wrench the robot applies to the environment in the
// sensor frame of the sensor task (MotionForceTask.cpp:793-828 read backwards), stored into that task's sensed rows.
// rd: a second wrench for the sensor, or NoReading; given (with a reading only): the frames of the final state, computed by
// the caller for its own report; without a reading they are computed here
template <class MD, class RD>
DI void contact_report(const MD& md, const DevParams& P, const Contact& ct, const real* q, const real* dq, int B, int b, const RD& rd,
					   const Frames* given) {
	Frames Fr;
	if constexpr (RD::on) {
		Fr = *given;
	} else {
		fk<true>(md, q, Fr);
	}
	real Rl[9], pl[3], xc[3], Rc[9];
	link_frame(P.contact_link, Fr, Rl, pl);
	const bool sensor = P.contact_sensor_task >= 0;
	if (sensor) {
		frame_pose(P.task[P.contact_sensor_task], Fr, xc, Rc);
	} else {
		UNROLL for (int a = 0; a < 3; a++) xc[a] = pl[a];
	}
	real Ft[3] = {0, 0, 0}, Mt[3] = {0, 0, 0};
	bool touching = false;
	UNROLL for (int k = 0; k < CONTACT_MAX_POINTS; k++) {
		real delta = 0, fn = 0;
		if (k < P.contact_n_points) {
			real x[3], Fk[3], m[3];
			contact_point(md, P, ct, Fr, Rl, pl, k, dq, x, Fk, delta, fn);
			const real r[3] = {x[0] - xc[0], x[1] - xc[1], x[2] - xc[2]};
			cross3(r, Fk, m);
			UNROLL for (int a = 0; a < 3; a++) {
				Ft[a] += Fk[a];
				Mt[a] += m[a];
			}
			touching = touching || fn > 0;
		}
		st(P.contact_status, k, B, b, delta);
		st(P.contact_status, CONTACT_MAX_POINTS + k, B, b, fn);
	}
	UNROLL for (int a = 0; a < 3; a++) {
		st(P.contact_status, 2 * CONTACT_MAX_POINTS + a, B, b, Ft[a]);
		st(P.contact_status, 2 * CONTACT_MAX_POINTS + 3 + a, B, b, Mt[a]);
	}
	const unsigned long long in_contact = __ballot(touching);
	if (threadIdx.x == 0 && in_contact) atomicAdd(P.contact_count, __popcll(in_contact));  // lane 0 always has a robot
	if (sensor) {
		if constexpr (RD::on) if (rd.add) {  // the external wrench on the same sensor: its moment about x_c joins the sum
			const real r[3] = {rd.x[0] - xc[0], rd.x[1] - xc[1], rd.x[2] - xc[2]};
			real m[3];
			cross3(r, rd.F, m);
			UNROLL for (int a = 0; a < 3; a++) {
				Ft[a] += rd.F[a];
				Mt[a] += rd.M[a] + m[a];
			}
		}
		const DevTask& t = P.task[P.contact_sensor_task];
		real Rs[9], os[3], ms_w[3], t1[3], fs[3], ms[3];
		mm<3, 3, 3>(Rc, t.sensor_rot, Rs);
		mv3(Rc, t.sensor_pos, os);	// o_s - x_c
		cross3(os, Ft, t1);
		// -sum (x_k - o_s) x F_k = -(sum (x_k - x_c) x F_k - (o_s - x_c) x sum F_k)
		UNROLL for (int a = 0; a < 3; a++) {
			ms_w[a] = t1[a] - Mt[a];
			t1[a] = -Ft[a];
		}
		mv_t<3, 3>(Rs, t1, fs);
		mv_t<3, 3>(Rs, ms_w, ms);
		UNROLL for (int a = 0; a < 3; a++) {
			st(t.sensed, a, B, b, fs[a]);
			st(t.sensed, 3 + a, B, b, ms[a]);
		}
	}
}

// ---- external wrench on a link of the plant (sai2b_set_external_wrench): a force F and a couple M per robot at point c of
// one link, for the robot's remaining `steps` periods.
// The law (DESIGN "External wrench on a link"), from the frames at the start of a substep:
//   x = p_l + R_l c,  F_w = F or R_l F,  M_w = M or R_l M,
//   tx_i = z_i . ((x - p_i) x F_w + M_w) revolute, z_i . F_w prismatic, for i <= link; 0 outboard and for an inactive robot
struct Wrench {
	real F[3], M[3], steps;	 // the robot's own rows of the [7][B] buffer
	bool active;			 // steps > 0 || steps < 0 on entry (a NaN: inactive)
};
DI void wrench_load(const WrenchParams& W, int B, int b, Wrench& wr) {
	UNROLL for (int k = 0; k < 3; k++) {
		wr.F[k] = ld(W.rows, k, B, b);
		wr.M[k] = ld(W.rows, 3 + k, B, b);
	}
	wr.steps = ld(W.rows, 6, B, b);
	wr.active = wr.steps > 0 || wr.steps < 0;
}
// x, F_w, M_w (zeros by select for an inactive robot) and tx in one pass over the joints; J is never formed
template <class MD>
DI void wrench_torques(const MD& md, const WrenchParams& W, const Wrench& wr, const Frames& Fr, real* x, real* Fw, real* Mw, real* tx) {
	real Rl[9], pl[3];
	link_frame(W.link, Fr, Rl, pl);
	const bool turn = W.frame != 0;	 // batch-uniform
	UNROLL for (int a = 0; a < 3; a++) {
		x[a] = fma(Rl[3 * a], W.point[0], fma(Rl[3 * a + 1], W.point[1], fma(Rl[3 * a + 2], W.point[2], pl[a])));
		const real f = turn ? fma(Rl[3 * a], wr.F[0], fma(Rl[3 * a + 1], wr.F[1], Rl[3 * a + 2] * wr.F[2])) : wr.F[a];
		const real m = turn ? fma(Rl[3 * a], wr.M[0], fma(Rl[3 * a + 1], wr.M[1], Rl[3 * a + 2] * wr.M[2])) : wr.M[a];
		Fw[a] = wr.active ? f : 0.0;
		Mw[a] = wr.active ? m : 0.0;
	}
	UNROLL for (int i = 0; i < N; i++) {
		const real z[3] = {Fr.R[i][2], Fr.R[i][5], Fr.R[i][8]};
		const real r[3] = {x[0] - Fr.p[i][0], x[1] - Fr.p[i][1], x[2] - Fr.p[i][2]};
		real m[3];
		cross3(r, Fw, m);
		UNROLL for (int a = 0; a < 3; a++) m[a] += Mw[a];
		const real* pr = (md.jtype[i] != 0) ? Fw : m;
		const real t = z[0] * pr[0] + z[1] * pr[1] + z[2] * pr[2];
		tx[i] = (i <= W.link && wr.active) ? t : 0.0;
	}
}
// After the last substep, from the frames of the final state: the status rows [6 + N][B] (F_w, M_w about x, tx), the count of
// robots pushed (one ballot, one atomic) and the countdown of `steps`; rd: what the sensor is to read
template <class MD>
DI void wrench_report(const MD& md, const WrenchParams& W, const Wrench& wr, const Frames& Fr, int B, int b, WrenchReading& rd) {
	real tx[N];
	wrench_torques(md, W, wr, Fr, rd.x, rd.F, rd.M, tx);
	UNROLL for (int a = 0; a < 3; a++) {
		st(W.status, a, B, b, rd.F[a]);
		st(W.status, 3 + a, B, b, rd.M[a]);
	}
	UNROLL for (int i = 0; i < N; i++) st(W.status, 6 + i, B, b, tx[i]);
	bool loaded = false;
	UNROLL for (int a = 0; a < 3; a++) loaded = loaded || wr.F[a] != 0.0 || wr.M[a] != 0.0;
	const unsigned long long pushed = __ballot(wr.active && loaded);
	if (threadIdx.x == 0 && pushed) atomicAdd(W.count, __popcll(pushed));  // lane 0 always has a robot
	st(W.rows, 6, B, b, wr.steps > 0 ? fmax(wr.steps - 1.0, 0.0) : wr.steps);
}
// what follows the last substep of a step with an external wrench: one fk for the wrench's report, the contact's and the sensor
template <class MD, class CT>
DI void wrench_finish(const MD& md, const DevParams& P, const WrenchParams& W, const Wrench& wr, const CT& ct, const real* q,
					  const real* dq, int B, int b) {
	Frames Fr;
	fk<true>(md, q, Fr);
	WrenchReading rd;
	wrench_report(md, W, wr, Fr, B, b, rd);
	rd.add = false;
	if constexpr (CT::on) {
		rd.add = W.sensor_task >= 0 && W.sensor_task == P.contact_sensor_task;
		contact_report(md, P, ct, q, dq, B, b, rd, &Fr);
	}
	if (W.sensor_task >= 0 && !rd.add) {
		real xc[3], Rc[9], m[3];
		frame_pose(P.task[W.sensor_task], Fr, xc, Rc);
		const real r[3] = {rd.x[0] - xc[0], rd.x[1] - xc[1], rd.x[2] - xc[2]};
		cross3(r, rd.F, m);
		UNROLL for (int a = 0; a < 3; a++) m[a] += rd.M[a];	 // about x_c
		sensor_store(P.task[W.sensor_task], Rc, rd.F, m, B, b);
	}
}

// PL: NoPayload / Payload (the PLANT's payload, sai2b_set_link_payload with SAI2B_PAYLOAD_PLANT), CT: NoContact / Contact;
// the host launches the instantiation for what the context has set, sim_kernel<NoPayload, NoContact> is the kernel without
// either feature.
// Every step body and report of this file works in coordinates whose origin is joint 0's frame (fk<true>): M, b, the lever
// arms, the moments about x_c and the sensor rows do not depend on the origin, mass_matrix's inertias about it stay the size
// of the robot however far the base stands from the world origin, and contact_load shifts the plane point to match.
// q_keep != NULL: the joint positions as they are on entry are saved there first (the pose the tasks cached at
// their last torque computation: see q_pose in sai2b_host.cpp)
template <class PL, class CT>
__global__ __launch_bounds__(64) void sim_kernel(const DevParams* __restrict__ Pp, const real* __restrict__ tau,
												 real dt, int substeps, int with_gravity, real* __restrict__ dbg_bias,
												 real* __restrict__ q_keep) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	real q[N], dq[N], tq[N];
	UNROLL for (int i = 0; i < N; i++) {
		q[i] = ld(P.q, i, B, b);
		dq[i] = ld(P.dq, i, B, b);
		tq[i] = tau ? ld(tau, i, B, b) : 0.0;
		if (q_keep) st(q_keep, i, B, b, q[i]);
	}
	[[maybe_unused]] PL pl;
	if constexpr (PL::on) payload_load(P.plant_payload, P.plant_payload_link, B, b, pl);
	[[maybe_unused]] CT ct;
	if constexpr (CT::on) contact_load(P.contact, P.model.xyz[0], B, b, ct);
	const real h = dt / substeps;
#pragma unroll 1
	for (int s = 0; s < substeps; s++) {
		Frames F;
		fk<true>(P.model, q, F);
		real M[N * N], L[N * N], dinv[N], bias[N], x[N];
		bias_forces(P.model, F, dq, with_gravity != 0, bias, pl);
		if (dbg_bias && s == 0) {
			UNROLL for (int i = 0; i < N; i++) st(dbg_bias, i, B, b, bias[i]);
		}
		mass_matrix(P.model, F, M, pl);
		chol<N>(M, L, dinv);
		if constexpr (CT::on) {
			real tc[N];
			contact_torques(P.model, P, ct, F, dq, tc);
			UNROLL for (int i = 0; i < N; i++) x[i] = (tq[i] + tc[i]) - bias[i];
		} else {
			UNROLL for (int i = 0; i < N; i++) x[i] = tq[i] - bias[i];
		}
		solve_lower<N>(L, dinv, x);
		solve_lower_t<N>(L, dinv, x);
		UNROLL for (int i = 0; i < N; i++) {
			dq[i] = fma(h, x[i], dq[i]);
			q[i] = fma(h, dq[i], q[i]);
		}
	}
	UNROLL for (int i = 0; i < N; i++) {
		st((real*)P.q, i, B, b, q[i]);
		st((real*)P.dq, i, B, b, dq[i]);
	}
	if constexpr (CT::on) contact_report(P.model, P, ct, q, dq, B, b, NoReading{}, nullptr);
}
// sim_kernel's step with the external wrench beside the contact torque: W by value as a kernel argument (batch-uniform, read
// with scalar loads). The step is written out a second time and sim_kernel is NOT an instantiation of a body shared with this
// one: behind one more level of inlining the compiler allocates and schedules the very same statements differently, and a
// context without a wrench must run the kernels it ran before the feature. A change to the step goes into both.
template <class PL, class CT>
__global__ __launch_bounds__(64) void sim_wrench_kernel(const DevParams* __restrict__ Pp, const real* __restrict__ tau, real dt, int substeps,
														int with_gravity, real* __restrict__ q_keep, const WrenchParams W) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	real q[N], dq[N], tq[N];
	UNROLL for (int i = 0; i < N; i++) {
		q[i] = ld(P.q, i, B, b);
		dq[i] = ld(P.dq, i, B, b);
		tq[i] = tau ? ld(tau, i, B, b) : 0.0;
		if (q_keep) st(q_keep, i, B, b, q[i]);
	}
	[[maybe_unused]] PL pl;
	if constexpr (PL::on) payload_load(P.plant_payload, P.plant_payload_link, B, b, pl);
	[[maybe_unused]] CT ct;
	if constexpr (CT::on) contact_load(P.contact, P.model.xyz[0], B, b, ct);
	Wrench wr;
	wrench_load(W, B, b, wr);
	const real h = dt / substeps;
#pragma unroll 1
	for (int s = 0; s < substeps; s++) {
		Frames F;
		fk<true>(P.model, q, F);
		real M[N * N], L[N * N], dinv[N], bias[N], x[N];
		bias_forces(P.model, F, dq, with_gravity != 0, bias, pl);
		mass_matrix(P.model, F, M, pl);
		chol<N>(M, L, dinv);
		real tx[N], xw[3], Fw[3], Mw[3];
		wrench_torques(P.model, W, wr, F, xw, Fw, Mw, tx);
		if constexpr (CT::on) {
			real tc[N];
			contact_torques(P.model, P, ct, F, dq, tc);
			UNROLL for (int i = 0; i < N; i++) x[i] = ((tq[i] + tc[i]) + tx[i]) - bias[i];
		} else {
			UNROLL for (int i = 0; i < N; i++) x[i] = (tq[i] + tx[i]) - bias[i];
		}
		solve_lower<N>(L, dinv, x);
		solve_lower_t<N>(L, dinv, x);
		UNROLL for (int i = 0; i < N; i++) {
			dq[i] = fma(h, x[i], dq[i]);
			q[i] = fma(h, dq[i], q[i]);
		}
	}
	UNROLL for (int i = 0; i < N; i++) {
		st((real*)P.q, i, B, b, q[i]);
		st((real*)P.dq, i, B, b, dq[i]);
	}
	wrench_finish(P.model, P, W, wr, ct, q, dq, B, b);
}

// ---- joint dynamics of the plant (sai2b_set_joint_dynamics): armature, damping, Coulomb friction, actuator saturation and
// joint stops, per robot and joint. The law (DESIGN "Joint dynamics in the simulated plant"), from the state at the start
// of a substep:
//   ts_i = min(max(tau_i, -t_i), t_i)
//   sl_i = max(0, k_i max(0, lo_i - q_i) (1 - c_i dq_i)),  su_i = max(0, k_i max(0, q_i - hi_i) (1 + c_i dq_i))
//   g_i  = d_i + f_i / sqrt(dq_i^2 + e_i^2)                 torque of damping + regularised Coulomb friction: -g_i dq_i
//   (M + diag(a) + h diag(g)) dq+ = (M + diag(a)) dq + h (ts + sl - su + tc - b),   q+ = q + h dq+
// continuous in the state everywhere; the dissipative term at the new velocity (linear-implicit), the stop spring explicit.
// Infinite limits give zero stop torques (max(0, -inf) = 0, k finite) and an infinite torque limit gives ts = tau.
struct JointRows {
	real a[N], d[N], f[N], lo[N], hi[N];  // the robot's own rows of the [6][N][B] buffer (the torque limit is used up on entry)
};
DI real joint_stop_torque(const JointParams& J, const JointRows& jr, int i, real q, real dq) {
	const real sl = fmax(0.0, J.stop_k[i] * fmax(0.0, jr.lo[i] - q) * (1.0 - J.stop_c[i] * dq));
	const real su = fmax(0.0, J.stop_k[i] * fmax(0.0, q - jr.hi[i]) * (1.0 + J.stop_c[i] * dq));
	return sl - su;
}
DI real joint_dissipation(const JointParams& J, const JointRows& jr, int i, real dq) {
	return jr.d[i] + jr.f[i] / sqrt(dq * dq + J.v_eps[i] * J.v_eps[i]);
}
// After the last substep: the status rows [3][N][B] (applied torque, stop torque and dissipative torque at the final state)
// and the two counters, one ballot and one atomic each
DI void joint_report(const JointParams& J, const JointRows& jr, const real* ts, bool saturated, const real* q, const real* dq, int B, int b) {
	bool at_stop = false;
	UNROLL for (int i = 0; i < N; i++) {
		const real s = joint_stop_torque(J, jr, i, q[i], dq[i]);
		at_stop = at_stop || s != 0.0;
		st(J.status, i, B, b, ts[i]);
		st(J.status, N + i, B, b, s);
		st(J.status, 2 * N + i, B, b, -joint_dissipation(J, jr, i, dq[i]) * dq[i]);
	}
	const unsigned long long sat = __ballot(saturated), stop = __ballot(at_stop);
	if (threadIdx.x == 0 && sat) atomicAdd(J.counts, __popcll(sat));  // lane 0 always has a robot
	if (threadIdx.x == 0 && stop) atomicAdd(J.counts + 1, __popcll(stop));
}

// sim_kernel's step with the joint terms: PL / CT as there, launched instead of it by a context that has joint dynamics set.
// a + h g goes on the diagonal ahead of the factorisation, (M + diag(a)) dq is formed from the unmodified M, and the two
// triangular solves return the new velocity itself.
template <class PL, class CT>
__global__ __launch_bounds__(64) void sim_joint_kernel(const DevParams* __restrict__ Pp, const real* __restrict__ tau, real dt, int substeps,
													   int with_gravity, real* __restrict__ q_keep, const JointParams J) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	real q[N], dq[N], ts[N];
	JointRows jr;
	bool saturated = false;
	UNROLL for (int i = 0; i < N; i++) {
		q[i] = ld(P.q, i, B, b);
		dq[i] = ld(P.dq, i, B, b);
		const real tq = tau ? ld(tau, i, B, b) : 0.0;
		if (q_keep) st(q_keep, i, B, b, q[i]);
		jr.a[i] = ld(J.rows, JOINT_ARMATURE * N + i, B, b);
		jr.d[i] = ld(J.rows, JOINT_DAMPING * N + i, B, b);
		jr.f[i] = ld(J.rows, JOINT_FRICTION * N + i, B, b);
		jr.lo[i] = ld(J.rows, JOINT_LOWER * N + i, B, b);
		jr.hi[i] = ld(J.rows, JOINT_UPPER * N + i, B, b);
		const real lim = ld(J.rows, JOINT_TORQUE_LIMIT * N + i, B, b);
		saturated = saturated || fabs(tq) > lim;
		ts[i] = fmin(fmax(tq, -lim), lim);
	}
	[[maybe_unused]] PL pl;
	if constexpr (PL::on) payload_load(P.plant_payload, P.plant_payload_link, B, b, pl);
	[[maybe_unused]] CT ct;
	if constexpr (CT::on) contact_load(P.contact, P.model.xyz[0], B, b, ct);
	const real h = dt / substeps;
#pragma unroll 1
	for (int s = 0; s < substeps; s++) {
		Frames F;
		fk<true>(P.model, q, F);
		real M[N * N], L[N * N], dinv[N], x[N];
		bias_forces(P.model, F, dq, with_gravity != 0, x, pl);
		if constexpr (CT::on) {
			real tc[N];
			contact_torques(P.model, P, ct, F, dq, tc);
			UNROLL for (int i = 0; i < N; i++) x[i] = ((ts[i] + joint_stop_torque(J, jr, i, q[i], dq[i])) + tc[i]) - x[i];
		} else {
			UNROLL for (int i = 0; i < N; i++) x[i] = (ts[i] + joint_stop_torque(J, jr, i, q[i], dq[i])) - x[i];
		}
		mass_matrix(P.model, F, M, pl);
		UNROLL for (int i = 0; i < N; i++) {
			real m = jr.a[i] * dq[i];
			UNROLL for (int j = 0; j < N; j++) m = fma(M[i * N + j], dq[j], m);
			x[i] = fma(h, x[i], m);
		}
		UNROLL for (int i = 0; i < N; i++) M[i * N + i] += fma(h, joint_dissipation(J, jr, i, dq[i]), jr.a[i]);
		chol<N>(M, L, dinv);
		solve_lower<N>(L, dinv, x);
		solve_lower_t<N>(L, dinv, x);
		UNROLL for (int i = 0; i < N; i++) {
			dq[i] = x[i];
			q[i] = fma(h, dq[i], q[i]);
		}
	}
	UNROLL for (int i = 0; i < N; i++) {
		st((real*)P.q, i, B, b, q[i]);
		st((real*)P.dq, i, B, b, dq[i]);
	}
	if constexpr (CT::on) contact_report(P.model, P, ct, q, dq, B, b, NoReading{}, nullptr);
	joint_report(J, jr, ts, saturated, q, dq, B, b);
}
// sim_joint_kernel's step with the external wrench, written out a second time for the reason given at sim_wrench_kernel
template <class PL, class CT>
__global__ __launch_bounds__(64) void sim_joint_wrench_kernel(const DevParams* __restrict__ Pp, const real* __restrict__ tau, real dt,
															  int substeps, int with_gravity, real* __restrict__ q_keep, const JointParams J,
															  const WrenchParams W) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	real q[N], dq[N], ts[N];
	JointRows jr;
	bool saturated = false;
	UNROLL for (int i = 0; i < N; i++) {
		q[i] = ld(P.q, i, B, b);
		dq[i] = ld(P.dq, i, B, b);
		const real tq = tau ? ld(tau, i, B, b) : 0.0;
		if (q_keep) st(q_keep, i, B, b, q[i]);
		jr.a[i] = ld(J.rows, JOINT_ARMATURE * N + i, B, b);
		jr.d[i] = ld(J.rows, JOINT_DAMPING * N + i, B, b);
		jr.f[i] = ld(J.rows, JOINT_FRICTION * N + i, B, b);
		jr.lo[i] = ld(J.rows, JOINT_LOWER * N + i, B, b);
		jr.hi[i] = ld(J.rows, JOINT_UPPER * N + i, B, b);
		const real lim = ld(J.rows, JOINT_TORQUE_LIMIT * N + i, B, b);
		saturated = saturated || fabs(tq) > lim;
		ts[i] = fmin(fmax(tq, -lim), lim);
	}
	[[maybe_unused]] PL pl;
	if constexpr (PL::on) payload_load(P.plant_payload, P.plant_payload_link, B, b, pl);
	[[maybe_unused]] CT ct;
	if constexpr (CT::on) contact_load(P.contact, P.model.xyz[0], B, b, ct);
	Wrench wr;
	wrench_load(W, B, b, wr);
	const real h = dt / substeps;
#pragma unroll 1
	for (int s = 0; s < substeps; s++) {
		Frames F;
		fk<true>(P.model, q, F);
		real M[N * N], L[N * N], dinv[N], x[N];
		bias_forces(P.model, F, dq, with_gravity != 0, x, pl);
		real tx[N], xw[3], Fw[3], Mw[3];
		wrench_torques(P.model, W, wr, F, xw, Fw, Mw, tx);
		if constexpr (CT::on) {
			real tc[N];
			contact_torques(P.model, P, ct, F, dq, tc);
			UNROLL for (int i = 0; i < N; i++) x[i] = (((ts[i] + joint_stop_torque(J, jr, i, q[i], dq[i])) + tc[i]) + tx[i]) - x[i];
		} else {
			UNROLL for (int i = 0; i < N; i++) x[i] = ((ts[i] + joint_stop_torque(J, jr, i, q[i], dq[i])) + tx[i]) - x[i];
		}
		mass_matrix(P.model, F, M, pl);
		UNROLL for (int i = 0; i < N; i++) {
			real m = jr.a[i] * dq[i];
			UNROLL for (int j = 0; j < N; j++) m = fma(M[i * N + j], dq[j], m);
			x[i] = fma(h, x[i], m);
		}
		UNROLL for (int i = 0; i < N; i++) M[i * N + i] += fma(h, joint_dissipation(J, jr, i, dq[i]), jr.a[i]);
		chol<N>(M, L, dinv);
		solve_lower<N>(L, dinv, x);
		solve_lower_t<N>(L, dinv, x);
		UNROLL for (int i = 0; i < N; i++) {
			dq[i] = x[i];
			q[i] = fma(h, dq[i], q[i]);
		}
	}
	UNROLL for (int i = 0; i < N; i++) {
		st((real*)P.q, i, B, b, q[i]);
		st((real*)P.dq, i, B, b, dq[i]);
	}
	wrench_finish(P.model, P, W, wr, ct, q, dq, B, b);
	joint_report(J, jr, ts, saturated, q, dq, B, b);
}

// ---- whole-arm contact of the plant (sai2b_set_body_contact): the collision configuration's link spheres pushed out of the
// robot's planes, its obstacle spheres and each other. The law is sai2b_body_contact_law.h (DESIGN "Whole-arm contact"); this file
// gives it the robot's sphere centres and link twists in per-lane LDS slots (slot s of lane t at [s * 64 + t]: a wavefront's
// lanes touch 512 contiguous bytes, and a lane reads what it wrote itself, so nothing is synchronised) and the joint axes
// from the frames.
// Centres: the frames live in registers under compile-time indices, so the link loop is unrolled and, inside it, a real loop
// over the spheres stores those that sit on the link (a scalar test on the by-value block). Twists about the origin of the
// coordinates: w_i and the velocity vo_i of frame i's origin run down the chain, v0_i = vo_i - w_i x p_i, and the material
// point of link i at c moves with v0_i + w_i x c, which is sum_{m <= i} dq_m z_m x (c - p_m) (dq_m z_m along a prismatic joint).
DI void body_fill(const DevModel& md, const BcGeom& G, const Frames& F, const real* dq, real* lds, real (&z)[N][3], real (&o)[N][3]) {
	real* xs = lds;
	real* tw = lds + (size_t)(3 * G.n_spheres) * 64;
#pragma unroll 1
	for (int k = 0; k < G.n_spheres; k++) {
		if (G.link[k] < 0) {  // a world point, in the step's coordinates
			UNROLL for (int a = 0; a < 3; a++) xs[(size_t)(3 * k + a) * 64] = G.centre[k][a] - md.xyz[0][a];
		}
	}
	real w[3] = {0, 0, 0}, vo[3] = {0, 0, 0};
	UNROLL for (int i = 0; i < N; i++) {
		const real* R = F.R[i];
		const real* p = F.p[i];
		UNROLL for (int a = 0; a < 3; a++) z[i][a] = R[3 * a + 2], o[i][a] = p[a];
		if (i > 0) {  // frame i's origin rides on link i - 1 (the world does not move)
			const real d[3] = {p[0] - F.p[i - 1][0], p[1] - F.p[i - 1][1], p[2] - F.p[i - 1][2]};
			real t[3];
			cross3(w, d, t);
			UNROLL for (int a = 0; a < 3; a++) vo[a] += t[a];
		}
		const bool pris = md.jtype[i] != 0;
		UNROLL for (int a = 0; a < 3; a++) {
			const real zq = z[i][a] * dq[i];
			vo[a] += pris ? zq : 0.0;
			w[a] += pris ? 0.0 : zq;
		}
		real t[3];
		cross3(w, p, t);
		UNROLL for (int a = 0; a < 3; a++) {
			tw[(size_t)(6 * i + a) * 64] = vo[a] - t[a];
			tw[(size_t)(6 * i + 3 + a) * 64] = w[a];
		}
#pragma unroll 1
		for (int k = 0; k < G.n_spheres; k++) {
			if (G.link[k] == i) {
				const double* c = G.centre[k];
				UNROLL for (int a = 0; a < 3; a++)
					xs[(size_t)(3 * k + a) * 64] = fma(R[3 * a], c[0], fma(R[3 * a + 1], c[1], fma(R[3 * a + 2], c[2], p[a])));
			}
		}
	}
}
// tb of the state the frames belong to; lds: the lane's first slot
DI void body_torques(const DevParams& P, const BodyParams& Bp, const Frames& F, const real* dq, real* lds, int B, int b, real k, real d,
					 real mu, real (&tb)[N]) {
	real z[N][3], o[N][3];
	body_fill(P.model, Bp.geom, F, dq, lds, z, o);
	body_contact_law<N, false>(Bp.geom, lds, lds + (size_t)(3 * Bp.geom.n_spheres) * 64, 64, z, o, P.model.jtype, P.model.xyz[0], Bp.env + b,
							   (size_t)B, k, d, mu, tb, nullptr);
}
// After the last substep, from the frames of the final state: the status rows [9 + N][B] (per category the deepest penetration,
// its witness, the sum of f_n; tb) and the four counters, one ballot and one atomic each
DI void body_report(const DevParams& P, const BodyParams& Bp, const real* q, const real* dq, real* lds, int B, int b, real k, real d, real mu) {
	Frames Fr;
	fk<true>(P.model, q, Fr);
	real z[N][3], o[N][3], tb[N];
	body_fill(P.model, Bp.geom, Fr, dq, lds, z, o);
	BcStatus s;
	body_contact_law<N, true>(Bp.geom, lds, lds + (size_t)(3 * Bp.geom.n_spheres) * 64, 64, z, o, P.model.jtype, P.model.xyz[0], Bp.env + b,
							  (size_t)B, k, d, mu, tb, &s);
	bool any = false;
	UNROLL for (int c = 0; c < COL_CATEGORIES; c++) {
		st(Bp.status, BC_DEPTH + c, B, b, s.depth[c]);
		st(Bp.status, BC_INDEX + c, B, b, (real)s.index[c]);
		st(Bp.status, BC_FSUM + c, B, b, s.fsum[c]);
		const bool touching = s.fsum[c] > 0.0;
		any = any || touching;
		const unsigned long long hit = __ballot(touching);
		if (threadIdx.x == 0 && hit) atomicAdd(Bp.counts + c, __popcll(hit));  // lane 0 always has a robot
	}
	UNROLL for (int i = 0; i < N; i++) st(Bp.status, BC_TORQUE + i, B, b, tb[i]);
	const unsigned long long hit = __ballot(any);
	if (threadIdx.x == 0 && hit) atomicAdd(Bp.counts + COL_CATEGORIES, __popcll(hit));
}

// The step of a context with whole-arm contact: PL / CT as everywhere, joint dynamics and the external wrench as run-time,
// batch-uniform switches (joint_on, wrench_on: scalar branches around the statements of sim_joint_kernel and sim_wrench_kernel),
// so that the feature adds four kernels per robot size, not sixteen. The four kernels above are not instantiations of this
// body, for the reason given at sim_wrench_kernel. tb joins the right-hand side beside tc and tx: explicit in the plain step,
// inside h (...) of the linear-implicit one, behind the torque limit. Dynamic LDS: 64 * bc_lds_slots(n_spheres, N) doubles.
template <class PL, class CT>
__global__ __launch_bounds__(64) void sim_body_kernel(const DevParams* __restrict__ Pp, const real* __restrict__ tau, real dt, int substeps,
													  int with_gravity, real* __restrict__ q_keep, const BodyParams Bp, const JointParams J,
													  const WrenchParams W, int joint_on, int wrench_on) {
	extern __shared__ real body_lds[];
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	real* lds = body_lds + threadIdx.x;
	real q[N], dq[N], ts[N];
	JointRows jr;
	bool saturated = false;
	UNROLL for (int i = 0; i < N; i++) {
		q[i] = ld(P.q, i, B, b);
		dq[i] = ld(P.dq, i, B, b);
		const real tq = tau ? ld(tau, i, B, b) : 0.0;
		if (q_keep) st(q_keep, i, B, b, q[i]);
		ts[i] = tq;
		jr.a[i] = jr.d[i] = jr.f[i] = 0.0;
		jr.lo[i] = -HUGE_VAL, jr.hi[i] = HUGE_VAL;
		if (joint_on) {
			jr.a[i] = ld(J.rows, JOINT_ARMATURE * N + i, B, b);
			jr.d[i] = ld(J.rows, JOINT_DAMPING * N + i, B, b);
			jr.f[i] = ld(J.rows, JOINT_FRICTION * N + i, B, b);
			jr.lo[i] = ld(J.rows, JOINT_LOWER * N + i, B, b);
			jr.hi[i] = ld(J.rows, JOINT_UPPER * N + i, B, b);
			const real lim = ld(J.rows, JOINT_TORQUE_LIMIT * N + i, B, b);
			saturated = saturated || fabs(tq) > lim;
			ts[i] = fmin(fmax(tq, -lim), lim);
		}
	}
	[[maybe_unused]] PL pl;
	if constexpr (PL::on) payload_load(P.plant_payload, P.plant_payload_link, B, b, pl);
	[[maybe_unused]] CT ct;
	if constexpr (CT::on) contact_load(P.contact, P.model.xyz[0], B, b, ct);
	Wrench wr;
	UNROLL for (int k = 0; k < 3; k++) wr.F[k] = wr.M[k] = 0.0;
	wr.steps = 0.0, wr.active = false;
	if (wrench_on) wrench_load(W, B, b, wr);
	const real bk = ld(Bp.rows, 0, B, b), bd = ld(Bp.rows, 1, B, b), bmu = ld(Bp.rows, 2, B, b);
	const real h = dt / substeps;
#pragma unroll 1
	for (int s = 0; s < substeps; s++) {
		Frames F;
		fk<true>(P.model, q, F);
		real M[N * N], L[N * N], dinv[N], x[N];
		bias_forces(P.model, F, dq, with_gravity != 0, x, pl);
		real tb[N];
		body_torques(P, Bp, F, dq, lds, B, b, bk, bd, bmu, tb);
		real tx[N];
		UNROLL for (int i = 0; i < N; i++) tx[i] = 0.0;
		if (wrench_on) {
			real xw[3], Fw[3], Mw[3];
			wrench_torques(P.model, W, wr, F, xw, Fw, Mw, tx);
		}
		if constexpr (CT::on) {
			real tc[N];
			contact_torques(P.model, P, ct, F, dq, tc);
			UNROLL for (int i = 0; i < N; i++) {
				const real stop = joint_on ? joint_stop_torque(J, jr, i, q[i], dq[i]) : 0.0;
				x[i] = ((((ts[i] + stop) + tc[i]) + tx[i]) + tb[i]) - x[i];
			}
		} else {
			UNROLL for (int i = 0; i < N; i++) {
				const real stop = joint_on ? joint_stop_torque(J, jr, i, q[i], dq[i]) : 0.0;
				x[i] = (((ts[i] + stop) + tx[i]) + tb[i]) - x[i];
			}
		}
		mass_matrix(P.model, F, M, pl);
		if (joint_on) {
			UNROLL for (int i = 0; i < N; i++) {
				real m = jr.a[i] * dq[i];
				UNROLL for (int j = 0; j < N; j++) m = fma(M[i * N + j], dq[j], m);
				x[i] = fma(h, x[i], m);
			}
			UNROLL for (int i = 0; i < N; i++) M[i * N + i] += fma(h, joint_dissipation(J, jr, i, dq[i]), jr.a[i]);
		}
		chol<N>(M, L, dinv);
		solve_lower<N>(L, dinv, x);
		solve_lower_t<N>(L, dinv, x);
		UNROLL for (int i = 0; i < N; i++) {
			dq[i] = joint_on ? x[i] : fma(h, x[i], dq[i]);
			q[i] = fma(h, dq[i], q[i]);
		}
	}
	UNROLL for (int i = 0; i < N; i++) {
		st((real*)P.q, i, B, b, q[i]);
		st((real*)P.dq, i, B, b, dq[i]);
	}
	if (wrench_on) {
		wrench_finish(P.model, P, W, wr, ct, q, dq, B, b);
	} else {
		if constexpr (CT::on) contact_report(P.model, P, ct, q, dq, B, b, NoReading{}, nullptr);
	}
	if (joint_on) joint_report(J, jr, ts, saturated, q, dq, B, b);
	body_report(P, Bp, q, dq, lds, B, b, bk, bd, bmu);
}

// What the tasks' observers read between ticks (MotionForceTask.h:121-165: getCurrentPosition /
// Orientation, getSensedForce/MomentControlWorldFrame; MotionForceTask.cpp:540-579: getPositionError,
// getOrientationError, goalPositionReached, goalOrientationReached), computed from the state and goal
// buffers as they are now. out [26][B]: position 3, orientation 9, sensed force 3 and moment 3 in the
// world frame at the control point, sigma_position (goal - current) 3, sigma_orientation orientationError 3,
// and the two scalar norms sqrt(e^T sigma e) the goal...Reached tests compare with their tolerance.
__global__ __launch_bounds__(64) void mft_status_kernel(const DevParams* __restrict__ Pp, int task, real* __restrict__ out) {
	const DevParams& P = *Pp;
	const int B = P.B;
	const int b = blockIdx.x * 64 + threadIdx.x;
	if (b >= B) return;
	const DevTask& t = P.task[task];
	real q[N], dq[N];
	UNROLL for (int i = 0; i < N; i++) {
		q[i] = ld(P.q, i, B, b);
		dq[i] = ld(P.dq, i, B, b);
	}
	Frames F;
	fk(P.model, q, F);
	real x[3], R[9];
	frame_pose(t, F, x, R);
	{  // getCurrentLinearVelocity / getCurrentAngularVelocity (MotionForceTask.h:127-146, MotionForceTask.cpp:293-298)
		real J[6 * N], v[6];
		jacobian(P.model, t, F, x, J);
		mv<6, N>(J, dq, v);
		UNROLL for (int k = 0; k < 6; k++) st(out, 26 + k, B, b, v[k]);
	}
	real sf[9], sp[9], sm[9], so[9];
	sigma_pair(t, 0, t.fdim, t.faxis, R, sf, sp);
	sigma_pair(t, 1, t.mdim, t.maxis, R, sm, so);
	real gpos[3], grot[9], e[3], oe[3], se[3], soe[3];
	UNROLL for (int k = 0; k < 3; k++) gpos[k] = ld(t.goals, k, B, b);
	UNROLL for (int k = 0; k < 9; k++) grot[k] = ld(t.goals, 3 + k, B, b);
	UNROLL for (int k = 0; k < 3; k++) e[k] = gpos[k] - x[k];
	orientation_error(grot, R, oe);
	mv3(sp, e, se);
	mv3(so, oe, soe);
	// sensed wrench at the control point, world frame (MotionForceTask.cpp:805-828)
	real sfc[3], smc[3], fs_w[3], ms_w[3];
	UNROLL for (int k = 0; k < 3; k++) {
		sfc[k] = ld(t.sensed, k, B, b);
		smc[k] = ld(t.sensed, 3 + k, B, b);
	}
	sensed_wrench_world(t, R, sfc, smc, fs_w, ms_w);
	UNROLL for (int k = 0; k < 3; k++) {
		st(out, k, B, b, x[k]);
		st(out, 12 + k, B, b, fs_w[k]);
		st(out, 15 + k, B, b, ms_w[k]);
		st(out, 18 + k, B, b, se[k]);
		st(out, 21 + k, B, b, soe[k]);
	}
	UNROLL for (int k = 0; k < 9; k++) {
		st(out, 3 + k, B, b, R[k]);
		// sigmaForce / sigmaPosition / sigmaMoment / sigmaOrientation (MotionForceTask.cpp:892-971)
		st(out, 32 + k, B, b, sf[k]);
		st(out, 41 + k, B, b, sp[k]);
		st(out, 50 + k, B, b, sm[k]);
		st(out, 59 + k, B, b, so[k]);
	}
	st(out, 24, B, b, sqrt(fmax(e[0] * se[0] + e[1] * se[1] + e[2] * se[2], 0.0)));
	st(out, 25, B, b, sqrt(fmax(oe[0] * soe[0] + oe[1] * soe[1] + oe[2] * soe[2], 0.0)));
}

int launch_mft_status(const DevParams* d_params, int B, int task, double* out, hipStream_t stream) {
	hipLaunchKernelGGL(mft_status_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_params, task, out);
	return launch_result();
}

int launch_sim(const DevParams* d_params, int B, const double* tau, double dt, int substeps, int with_gravity, bool payload, bool contact,
			   const JointParams* joint, const WrenchParams* wrench, const BodyParams* body, double* dbg_bias, double* q_keep, hipStream_t stream) {
	const dim3 grid((B + 63) / 64), block(64);
	if (body) {	 // whole-arm contact: one kernel for every form, joint dynamics and the wrench as its run-time switches
		if (dbg_bias) return 1;
		static constexpr decltype(&sim_body_kernel<NoPayload, NoContact>) body_kernel[2][2] = {
			{sim_body_kernel<NoPayload, NoContact>, sim_body_kernel<Payload, NoContact>},
			{sim_body_kernel<NoPayload, Contact>, sim_body_kernel<Payload, Contact>}};
		const size_t lds = (size_t)64 * bc_lds_slots(body->geom.n_spheres, N) * sizeof(double);
		hipLaunchKernelGGL(body_kernel[contact][payload], grid, block, lds, stream, d_params, tau, dt, substeps, with_gravity, q_keep, *body,
						   joint ? *joint : JointParams{}, wrench ? *wrench : WrenchParams{}, joint ? 1 : 0, wrench ? 1 : 0);
		return launch_result();
	}
	if (wrench) {  // the forms with an external wrench (dbg_bias: sai2b_get_bias never sees one)
		if (dbg_bias) return 1;
		if (joint) {
			static constexpr decltype(&sim_joint_wrench_kernel<NoPayload, NoContact>) joint_wrench_kernel[2][2] = {
				{sim_joint_wrench_kernel<NoPayload, NoContact>, sim_joint_wrench_kernel<Payload, NoContact>},
				{sim_joint_wrench_kernel<NoPayload, Contact>, sim_joint_wrench_kernel<Payload, Contact>}};
			hipLaunchKernelGGL(joint_wrench_kernel[contact][payload], grid, block, 0, stream, d_params, tau, dt, substeps, with_gravity, q_keep,
							   *joint, *wrench);
			return launch_result();
		}
		static constexpr decltype(&sim_wrench_kernel<NoPayload, NoContact>) wrench_kernel[2][2] = {
			{sim_wrench_kernel<NoPayload, NoContact>, sim_wrench_kernel<Payload, NoContact>},
			{sim_wrench_kernel<NoPayload, Contact>, sim_wrench_kernel<Payload, Contact>}};
		hipLaunchKernelGGL(wrench_kernel[contact][payload], grid, block, 0, stream, d_params, tau, dt, substeps, with_gravity, q_keep, *wrench);
		return launch_result();
	}
	if (joint) {
		static constexpr decltype(&sim_joint_kernel<NoPayload, NoContact>) joint_kernel[2][2] = {
			{sim_joint_kernel<NoPayload, NoContact>, sim_joint_kernel<Payload, NoContact>},
			{sim_joint_kernel<NoPayload, Contact>, sim_joint_kernel<Payload, Contact>}};
		if (dbg_bias) return 1;
		hipLaunchKernelGGL(joint_kernel[contact][payload], dim3((B + 63) / 64), dim3(64), 0, stream, d_params, tau, dt, substeps, with_gravity,
						   q_keep, *joint);
		return launch_result();
	}
	static constexpr decltype(&sim_kernel<NoPayload, NoContact>) kernel[2][2] = {
		{sim_kernel<NoPayload, NoContact>, sim_kernel<Payload, NoContact>}, {sim_kernel<NoPayload, Contact>, sim_kernel<Payload, Contact>}};
	hipLaunchKernelGGL(kernel[contact][payload], dim3((B + 63) / 64), dim3(64), 0, stream, d_params, tau, dt, substeps, with_gravity, dbg_bias,
					   q_keep);
	return launch_result();
}

}  // namespace sai2b

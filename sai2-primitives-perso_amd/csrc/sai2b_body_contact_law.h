// sai2b_body_contact_law.h — whole-arm contact of the simulated plant (include/sai2b.h "whole-arm contact"): the link spheres of
// the collision configuration pushed out of the robot's planes, its obstacle spheres and each other by the contact law of the
// plant (sai2b_sim.hip, "contact of the plant"). Per robot: the joint torques tb of every penetrating candidate and, when asked,
// the status (per category the deepest penetration, its witness and the sum of the normal forces). A pure function of the
// batch-uniform geometry, the robot's sphere centres, link twists and joint axes, and its rows, so sim_body_kernel (sai2b_sim.hip)
// and a CPU program (tests/cpp/body_contact_driver.cpp) run the same code. No HIP in here when a host compiler reads it.
//
// Written for one lane per robot inside a loop that runs every substep, so unlike sai2b_collision_law.h nothing here is unrolled
// over spheres or pairs: the loops over spheres, planes, obstacles and partners are real loops (`unroll 1` on the device) over
// the batch-uniform block, the sphere centres and the link twists are read at run-time indices from per-lane slots of a buffer
// with a stride (LDS on the device: slot s of lane t at [s * 64 + t]; the CPU program: stride 1), and private arrays are indexed
// by compile-time constants only (the 3 components and, unrolled, the DOF joints). What a candidate costs beyond its
// penetration test is skipped by the whole wavefront when none of its lanes penetrates.
//
// Sphere-centric: sphere a gathers the force of every plane, obstacle and partner sphere on itself, F_a and the moment n_a of
// those forces about its own centre x_a, and is projected onto the joints once: tb_m += z_m . (n_a + (x_a - o_m) x F_a) about a
// revolute joint m <= link(a), z_m . F_a along a prismatic one. A self pair (i, j) is therefore evaluated twice, always in the
// order (i, j) of the law (u = (x_i - x_j) / |x_i - x_j|), so that the force on j is the exact negative of the force on i.
#pragma once
#include <cmath>
#include <cstddef>

#include "sai2b_collision_law.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define SAI2B_BC_LOOP _Pragma("unroll 1")
#define SAI2B_BC_ANY(p) (__ballot(p) != 0ull)
#else
#define SAI2B_BC_LOOP
#define SAI2B_BC_ANY(p) (p)
#endif

namespace sai2b {

constexpr int BC_ROWS = 3;	  // per robot: stiffness k, damping d, friction mu
constexpr int BC_COUNTS = 4;  // robots with some f_n > 0 in plane, obstacle, self; in any
constexpr int BC_DEPTH = 0, BC_INDEX = 3, BC_FSUM = 6, BC_TORQUE = 9;  // first rows of the status [9 + dof][B]
constexpr int bc_status_rows(int dof) { return BC_TORQUE + dof; }
constexpr int bc_lds_slots(int n_spheres, int dof) { return 3 * n_spheres + 6 * dof; }	// doubles per lane: centres, link twists

// the batch-uniform part: the collision configuration's spheres and masks, the categories in force and the friction regularisation
struct BcGeom {
	int n_spheres, n_planes, n_obstacles;
	int categories;	 // bit c: category c (COL_PLANE, COL_OBSTACLE, COL_SELF) pushes
	unsigned env_mask;
	unsigned partner[COL_MAX_SPHERES];	// bit b of partner[a]: a and b are a tested pair, in either order (the symmetric pair_mask)
	int link[COL_MAX_SPHERES];
	double centre[COL_MAX_SPHERES][3], radius[COL_MAX_SPHERES];
	double v_eps;
};

struct BcStatus {
	double depth[COL_CATEGORIES];  // the deepest max(0, delta), 0 without a penetration
	int index[COL_CATEGORIES];	   // its witness in the collision's encoding (16 p + k, 16 o + k, 16 i + j), -1 without one
	double fsum[COL_CATEGORIES];   // sum of f_n
};

// The force of one candidate ON the body whose point moves with v relative to the other side, u pointing out of the other side:
// the plant's contact law term for term. Returns f_n. A NaN delta gives f_n = 0 (fmax drops the NaN) and F = 0.
SAI2B_COL_HD inline double bc_force(const double u[3], double delta, const double v[3], double k, double d, double mu, double v_eps, double F[3]) {
	const double vn = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
	const double fn = fmax(0.0, k * fmax(0.0, delta) * (1.0 - d * vn));
	const double vt[3] = {v[0] - vn * u[0], v[1] - vn * u[1], v[2] - vn * u[2]};
	const double s = mu * fn / sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2] + v_eps * v_eps);
	const bool on = fn > 0.0;  // false for a NaN
	F[0] = on ? fn * u[0] - s * vt[0] : 0.0, F[1] = on ? fn * u[1] - s * vt[1] : 0.0, F[2] = on ? fn * u[2] - s * vt[2] : 0.0;
	return on ? fn : 0.0;
}

// velocity of the material point of link l at c: v0_l + w_l x c from the link's twist about the origin (link -1: the world, 0)
SAI2B_COL_HD inline void bc_point_velocity(const double* tw, size_t S, int l, const double c[3], double v[3]) {
	v[0] = v[1] = v[2] = 0.0;
	if (l >= 0) {
		const double* t = tw + (size_t)(6 * l) * S;
		const double w0 = t[3 * S], w1 = t[4 * S], w2 = t[5 * S];
		v[0] = t[0] + (w1 * c[2] - w2 * c[1]);
		v[1] = t[S] + (w2 * c[0] - w0 * c[2]);
		v[2] = t[2 * S] + (w0 * c[1] - w1 * c[0]);
	}
}

// deeper, or as deep with the smaller index (the first in the collision's loop order); a delta that is not > 0 never wins
SAI2B_COL_HD inline void bc_note(BcStatus* st, int cat, double delta, int idx, double fn) {
	const bool wins = delta > st->depth[cat] || (delta > 0.0 && delta == st->depth[cat] && idx < st->index[cat]);
	st->depth[cat] = wins ? delta : st->depth[cat];
	st->index[cat] = wins ? idx : st->index[cat];
	st->fsum[cat] += fn;
}

// One robot. xs: its sphere centres, slot 3 k + a; tw: its link twists, slot 6 l + (v0 3, w 3); both with stride S, in coordinates
// whose origin stands at `origin` in the world (the environment rows are world rows and are shifted by it); z, o: axis and origin
// of every joint frame in those coordinates; env: its rows of the collision's environment with stride sB (not read without a plane
// and an obstacle); k, d, mu: its rows. tb: the joint torques; st (STATUS): the status.
template <int DOF, bool STATUS>
SAI2B_COL_HD inline void body_contact_law(const BcGeom& G, const double* xs, const double* tw, size_t S, const double (&z)[DOF][3],
										   const double (&o)[DOF][3], const int* jtype, const double* origin, const double* env, size_t sB,
										   double k, double d, double mu, double (&tb)[DOF], BcStatus* st) {
	SAI2B_COL_UNROLL
	for (int m = 0; m < DOF; m++) tb[m] = 0.0;
	if (STATUS) {
		SAI2B_COL_UNROLL
		for (int c = 0; c < COL_CATEGORIES; c++) st->depth[c] = 0.0, st->index[c] = -1, st->fsum[c] = 0.0;
	}
	// rows that are not all >= 0 (a NaN compares false): the robot feels nothing; the status still reports its penetrations
	const bool rows_ok = k >= 0.0 && d >= 0.0 && mu >= 0.0;
	if (!STATUS && !SAI2B_BC_ANY(rows_ok && k > 0.0)) return;
	const double kk = rows_ok ? k : 0.0, dd = rows_ok ? d : 0.0, mm_ = rows_ok ? mu : 0.0;
	const int obstacle_base = COL_PLANE_ROWS * G.n_planes;
	SAI2B_BC_LOOP
	for (int a = 0; a < G.n_spheres; a++) {
		const int la = G.link[a];
		const double ra = G.radius[a];
		const double xa[3] = {xs[(size_t)(3 * a) * S], xs[(size_t)(3 * a + 1) * S], xs[(size_t)(3 * a + 2) * S]};
		double Fa[3] = {0, 0, 0}, na[3] = {0, 0, 0};
		bool hit = false;
		// F at x_a + s u on sphere a: the moment is taken about the sphere's own centre, where the lever is the radius, and carried
		// to the joints with the lever x_a - o_m below; a candidate without a force adds nothing, whatever its point holds (an
		// absent plane's is a NaN)
		auto apply = [&](const double F[3], const double u[3], double s, bool on) {
			Fa[0] += on ? F[0] : 0.0, Fa[1] += on ? F[1] : 0.0, Fa[2] += on ? F[2] : 0.0;
			na[0] += on ? s * (u[1] * F[2] - u[2] * F[1]) : 0.0, na[1] += on ? s * (u[2] * F[0] - u[0] * F[2]) : 0.0,
				na[2] += on ? s * (u[0] * F[1] - u[1] * F[0]) : 0.0;
			hit = hit || on;
		};
		if ((G.env_mask >> a) & 1) {
			if (G.categories & (1 << COL_PLANE)) {
				SAI2B_BC_LOOP
				for (int p = 0; p < G.n_planes; p++) {
					const double* w = env + (size_t)(COL_PLANE_ROWS * p) * sB;
					const double u[3] = {w[3 * sB], w[4 * sB], w[5 * sB]};
					const double delta =
						ra - (u[0] * (xa[0] - (w[0] - origin[0])) + u[1] * (xa[1] - (w[sB] - origin[1])) + u[2] * (xa[2] - (w[2 * sB] - origin[2])));
					if (SAI2B_BC_ANY(delta > 0.0)) {
						const double c[3] = {xa[0] - ra * u[0], xa[1] - ra * u[1], xa[2] - ra * u[2]};
						double v[3], F[3];
						bc_point_velocity(tw, S, la, c, v);
						const double fn = bc_force(u, delta, v, kk, dd, mm_, G.v_eps, F);
						apply(F, u, -ra, fn > 0.0);
						if (STATUS) bc_note(st, COL_PLANE, delta, 16 * p + a, fn);
					}
				}
			}
			if (G.categories & (1 << COL_OBSTACLE)) {
				SAI2B_BC_LOOP
				for (int ob = 0; ob < G.n_obstacles; ob++) {
					const double* w = env + (size_t)(obstacle_base + COL_OBSTACLE_ROWS * ob) * sB;
					const double e[3] = {xa[0] - (w[0] - origin[0]), xa[1] - (w[sB] - origin[1]), xa[2] - (w[2 * sB] - origin[2])};
					const double e2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], rr = ra + w[3 * sB];
					// a superset of delta > 0 without the root (a NaN anywhere: false); delta itself decides below
					if (SAI2B_BC_ANY(e2 < rr * rr * (1.0 + 1e-9) && e2 > 0.0)) {
						const double len = sqrt(e2);
						const bool some = len > 0.0;
						const double inv = some ? 1.0 / len : 0.0;
						const double u[3] = {e[0] * inv, e[1] * inv, e[2] * inv};
						const double delta = some ? rr - len : 0.0;
						const double c[3] = {xa[0] - ra * u[0], xa[1] - ra * u[1], xa[2] - ra * u[2]};
						double v[3], F[3];
						bc_point_velocity(tw, S, la, c, v);
						const double fn = bc_force(u, delta, v, kk, dd, mm_, G.v_eps, F);
						apply(F, u, -ra, fn > 0.0);
						if (STATUS) bc_note(st, COL_OBSTACLE, delta, 16 * ob + a, fn);
					}
				}
			}
		}
		if (G.categories & (1 << COL_SELF)) {
			const unsigned partners = G.partner[a];
			SAI2B_BC_LOOP
			for (int b = 0; b < G.n_spheres; b++) {
				if (!((partners >> b) & 1)) continue;
				const bool first = a < b;  // a is the pair's i
				const int lb = G.link[b];
				const double rb = G.radius[b];
				const double xb[3] = {xs[(size_t)(3 * b) * S], xs[(size_t)(3 * b + 1) * S], xs[(size_t)(3 * b + 2) * S]};
				// the pair as the law writes it: (i, j) with i < j
				const double e[3] = {first ? xa[0] - xb[0] : xb[0] - xa[0], first ? xa[1] - xb[1] : xb[1] - xa[1], first ? xa[2] - xb[2] : xb[2] - xa[2]};
				const double e2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], rr = ra + rb;
				if (SAI2B_BC_ANY(e2 < rr * rr * (1.0 + 1e-9) && e2 > 0.0)) {
					const double len = sqrt(e2);
					const bool some = len > 0.0;
					const double inv = some ? 1.0 / len : 0.0;
					const double u[3] = {e[0] * inv, e[1] * inv, e[2] * inv};
					const double delta = some ? rr - len : 0.0;
					const double sa = first ? -ra : ra, sb = first ? rb : -rb;	// c_i = x_i - r_i u, c_j = x_j + r_j u
					const double ca[3] = {xa[0] + sa * u[0], xa[1] + sa * u[1], xa[2] + sa * u[2]};
					const double cb[3] = {xb[0] + sb * u[0], xb[1] + sb * u[1], xb[2] + sb * u[2]};
					double va[3], vb[3], F[3];
					bc_point_velocity(tw, S, la, ca, va);
					bc_point_velocity(tw, S, lb, cb, vb);
					const double vrel[3] = {first ? va[0] - vb[0] : vb[0] - va[0], first ? va[1] - vb[1] : vb[1] - va[1],
											first ? va[2] - vb[2] : vb[2] - va[2]};	 // v(c_i) - v(c_j)
					const double fn = bc_force(u, delta, vrel, kk, dd, mm_, G.v_eps, F);  // on i; j feels -F
					const double Fa_[3] = {first ? F[0] : -F[0], first ? F[1] : -F[1], first ? F[2] : -F[2]};
					apply(Fa_, u, sa, fn > 0.0);
					if (STATUS && first) bc_note(st, COL_SELF, delta, 16 * a + b, fn);
				}
			}
		}
		if (la >= 0 && SAI2B_BC_ANY(hit)) {
			SAI2B_COL_UNROLL
			for (int m = 0; m < DOF; m++) {
				const double l0 = xa[0] - o[m][0], l1 = xa[1] - o[m][1], l2 = xa[2] - o[m][2];
				const double r0 = na[0] + (l1 * Fa[2] - l2 * Fa[1]), r1 = na[1] + (l2 * Fa[0] - l0 * Fa[2]), r2 = na[2] + (l0 * Fa[1] - l1 * Fa[0]);
				const double t = jtype[m] ? z[m][0] * Fa[0] + z[m][1] * Fa[1] + z[m][2] * Fa[2] : z[m][0] * r0 + z[m][1] * r1 + z[m][2] * r2;
				tb[m] += (m <= la && hit) ? t : 0.0;
			}
		}
	}
}

// ---- for CPU programs: the chain of sai2b_collision_law.h (convention of include/sai2b_detfk.h) carried to what the law takes.
// Plain FP64 in world coordinates (origin 0): z_m, o_m, the sphere centres xs [3 n_spheres] and the link twists tw [6 DOF]
// about the world origin, stride 1. E [DOF][9], xyz [DOF][3], jtype [DOF] as ColLaw holds them.
template <int DOF>
inline void bc_host_kinematics(const BcGeom& G, const double* E, const double* xyz, const int* jtype, const double* q, const double* dq,
							   double (&z)[DOF][3], double (&o)[DOF][3], double* xs, double* tw) {
	double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0}, w[3] = {0, 0, 0}, vo[3] = {0, 0, 0};
	for (int k = 0; k < G.n_spheres; k++)
		for (int a = 0; a < 3; a++) xs[3 * k + a] = G.link[k] < 0 ? G.centre[k][a] : 0.0;
	for (int i = 0; i < DOF; i++) {
		double RE[9], pn[3];
		for (int r = 0; r < 3; r++) {
			pn[r] = p[r] + (R[3 * r] * xyz[3 * i] + R[3 * r + 1] * xyz[3 * i + 1] + R[3 * r + 2] * xyz[3 * i + 2]);
			for (int c = 0; c < 3; c++) RE[3 * r + c] = R[3 * r] * E[9 * i + c] + R[3 * r + 1] * E[9 * i + 3 + c] + R[3 * r + 2] * E[9 * i + 6 + c];
		}
		if (jtype[i]) {
			for (int r = 0; r < 3; r++) pn[r] += RE[3 * r + 2] * q[i];
			for (int r = 0; r < 9; r++) R[r] = RE[r];
		} else {
			const double s = sin(q[i]), c = cos(q[i]);
			for (int r = 0; r < 3; r++) {
				R[3 * r] = c * RE[3 * r] + s * RE[3 * r + 1];
				R[3 * r + 1] = c * RE[3 * r + 1] - s * RE[3 * r];
				R[3 * r + 2] = RE[3 * r + 2];
			}
		}
		// the origin of frame i rides on link i - 1 and, along a prismatic joint, slides with dq_i
		const double d[3] = {pn[0] - p[0], pn[1] - p[1], pn[2] - p[2]};
		vo[0] += w[1] * d[2] - w[2] * d[1], vo[1] += w[2] * d[0] - w[0] * d[2], vo[2] += w[0] * d[1] - w[1] * d[0];
		for (int r = 0; r < 3; r++) {
			p[r] = pn[r];
			z[i][r] = R[3 * r + 2], o[i][r] = p[r];
			if (jtype[i])
				vo[r] += z[i][r] * dq[i];
			else
				w[r] += z[i][r] * dq[i];
		}
		tw[6 * i] = vo[0] - (w[1] * p[2] - w[2] * p[1]);
		tw[6 * i + 1] = vo[1] - (w[2] * p[0] - w[0] * p[2]);
		tw[6 * i + 2] = vo[2] - (w[0] * p[1] - w[1] * p[0]);
		for (int r = 0; r < 3; r++) tw[6 * i + 3 + r] = w[r];
		for (int k = 0; k < G.n_spheres; k++)
			if (G.link[k] == i)
				for (int r = 0; r < 3; r++) xs[3 * k + r] = p[r] + (R[3 * r] * G.centre[k][0] + R[3 * r + 1] * G.centre[k][1] + R[3 * r + 2] * G.centre[k][2]);
	}
}

}  // namespace sai2b

// sai2b_collision_law.h — the proximity of one robot to its environment and to itself (include/sai2b.h "collision proximity"):
// spheres fixed to the links against per-robot planes and obstacle spheres and against each other; per category the smallest
// distance with its witness (index, normal) and its gradient with respect to q, the flags byte, and the world centres. A pure
// function of the batch-uniform geometry, the robot's q and its environment rows, so collision_kernel (sai2b_collision.hip) and
// a CPU program (tests/cpp/collision_driver.cpp) run the same code. No HIP in here when a host compiler reads it.
// Every buffer is [row][stride]: the kernel passes its column (base + b) with stride B, the CPU program a robot of its own with
// stride 1.
// Written for one lane per robot: every array is indexed by loop counters that are compile-time constants once the loops are
// unrolled (the device build unrolls all of them), so nothing goes to scratch. What is batch-uniform but not known at compile time
// (which link a sphere sits on, which pairs are tested) is a wave-uniform test on the by-value block around straight-line code;
// what differs per lane (which sphere won) is a select over the compile-time index, never an index.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define SAI2B_COL_HD __host__ __device__
#else
#define SAI2B_COL_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SAI2B_COL_UNROLL _Pragma("unroll")
#else
#define SAI2B_COL_UNROLL
#endif

namespace sai2b {

constexpr int COL_MAX_SPHERES = 16, COL_MAX_PLANES = 2, COL_MAX_OBSTACLES = 4;	// SAI2B_MAX_COLLISION_*
constexpr int COL_PLANE_ROWS = 6, COL_OBSTACLE_ROWS = 4;						// point 3, normal 3; centre 3, radius
constexpr int COL_ENV_ROWS_MAX = COL_PLANE_ROWS * COL_MAX_PLANES + COL_OBSTACLE_ROWS * COL_MAX_OBSTACLES;
constexpr int COL_CATEGORIES = 3;  // plane, obstacle, self
enum { COL_PLANE = 0, COL_OBSTACLE = 1, COL_SELF = 2 };
enum { COL_DISTANCE = 1, COL_INDEX = 2, COL_NORMAL = 4, COL_GRADIENT = 8, COL_CENTRES = 16, COL_ALL_BLOCKS = 31 };  // SAI2B_COL_*
constexpr int COL_BLOCKS = 5;
enum { COL_FLAG_PLANE = 1, COL_FLAG_OBSTACLE = 2, COL_FLAG_SELF = 4, COL_FLAG_NONFINITE = 8 };
constexpr int COL_COUNTS = 5;  // robots per flag bit, robots with a non-zero byte

constexpr int col_env_rows(int n_planes, int n_obstacles) { return COL_PLANE_ROWS * n_planes + COL_OBSTACLE_ROWS * n_obstacles; }
// rows of one block: per category 1, 1, 3, dof; the centres 3 per sphere
constexpr int col_block_rows(int block, int dof, int n_spheres) {
	return block == COL_DISTANCE || block == COL_INDEX ? COL_CATEGORIES
		   : block == COL_NORMAL					   ? 3 * COL_CATEGORIES
		   : block == COL_GRADIENT					   ? dof * COL_CATEGORIES
		   : block == COL_CENTRES					   ? 3 * n_spheres
													   : 0;
}
// first row of every block in flag order (-1: not selected); returns the rows of the whole output
inline int col_layout(int blocks, int dof, int n_spheres, int row[COL_BLOCKS]) {
	int rows = 0;
	for (int k = 0; k < COL_BLOCKS; k++) {
		const bool on = (blocks >> k) & 1;
		row[k] = on ? rows : -1;
		if (on) rows += col_block_rows(1 << k, dof, n_spheres);
	}
	return rows;
}

// the batch-uniform part: the chain (convention of include/sai2b_detfk.h), the spheres, the masks, the margins and the layout
template <int DOF>
struct ColLaw {
	double E[DOF][9], xyz[DOF][3];	// joint frame in the parent link
	int jtype[DOF];					// 0 revolute about, 1 prismatic along the joint frame's z
	int n_spheres, n_planes, n_obstacles, blocks;
	unsigned env_mask;
	unsigned pair_mask[COL_MAX_SPHERES];
	int link[COL_MAX_SPHERES];
	double centre[COL_MAX_SPHERES][3], radius[COL_MAX_SPHERES];
	double margin[COL_CATEGORIES];
	int row[COL_BLOCKS];  // first row of DISTANCE, INDEX, NORMAL, GRADIENT, CENTRES in the output, -1: not stored
};

SAI2B_COL_HD inline bool col_finite(double v) { return v - v == 0.0; }

// u . d x / d q_m for a point x on link `lx`, every m: z_m x (x - o_m) about a revolute joint, z_m along a prismatic one,
// zero beyond the point's link (a per-lane select on the compile-time m)
template <int DOF>
SAI2B_COL_HD inline void col_gradient(const ColLaw<DOF>& G, const double (&z)[DOF][3], const double (&o)[DOF][3], const double u[3],
									   const double x[3], int lx, double sign, double g[DOF]) {
	SAI2B_COL_UNROLL
	for (int m = 0; m < DOF; m++) {
		double v;
		if (G.jtype[m]) {
			v = u[0] * z[m][0] + u[1] * z[m][1] + u[2] * z[m][2];
		} else {
			const double r0 = x[0] - o[m][0], r1 = x[1] - o[m][1], r2 = x[2] - o[m][2];
			v = u[0] * (z[m][1] * r2 - z[m][2] * r1) + u[1] * (z[m][2] * r0 - z[m][0] * r2) + u[2] * (z[m][0] * r1 - z[m][1] * r0);
		}
		g[m] += m <= lx ? sign * v : 0.0;
	}
}

// One robot. q: its joint positions; env: its environment rows (not read when there is no plane and no obstacle); out: its column
// of the output or NULL. Returns the flags byte.
template <int DOF>
SAI2B_COL_HD inline int collision_law(const ColLaw<DOF>& G, const double* q, const double* env, size_t sB, double* out) {
	const double inf = HUGE_VAL;
	const int blocks = out ? G.blocks : 0;
	const bool want_normal = (blocks & (COL_NORMAL | COL_GRADIENT)) != 0, want_gradient = (blocks & COL_GRADIENT) != 0;
	// ---- forward kinematics: z_m and o_m of every joint, the centre of every sphere behind its link's frame
	double z[DOF][3], o[DOF][3], x[COL_MAX_SPHERES][3];
	double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
	bool finite = true;
	SAI2B_COL_UNROLL
	for (int k = 0; k < COL_MAX_SPHERES; k++) {
		const bool world = k < G.n_spheres && G.link[k] < 0;
		SAI2B_COL_UNROLL
		for (int a = 0; a < 3; a++) x[k][a] = world ? G.centre[k][a] : 0.0;
	}
	SAI2B_COL_UNROLL
	for (int i = 0; i < DOF; i++) {
		const double qi = q[(size_t)i * sB];
		finite = finite && col_finite(qi);
		double RE[9];
		SAI2B_COL_UNROLL
		for (int r = 0; r < 3; r++) {
			p[r] = p[r] + (R[3 * r] * G.xyz[i][0] + R[3 * r + 1] * G.xyz[i][1] + R[3 * r + 2] * G.xyz[i][2]);
			SAI2B_COL_UNROLL
			for (int c = 0; c < 3; c++) RE[3 * r + c] = R[3 * r] * G.E[i][c] + R[3 * r + 1] * G.E[i][3 + c] + R[3 * r + 2] * G.E[i][6 + c];
		}
		if (G.jtype[i]) {
			SAI2B_COL_UNROLL
			for (int r = 0; r < 3; r++) {
				p[r] = p[r] + RE[3 * r + 2] * qi;
				R[3 * r] = RE[3 * r], R[3 * r + 1] = RE[3 * r + 1], R[3 * r + 2] = RE[3 * r + 2];
			}
		} else {
			const double s = sin(qi), c = cos(qi);
			SAI2B_COL_UNROLL
			for (int r = 0; r < 3; r++) {
				R[3 * r] = c * RE[3 * r] + s * RE[3 * r + 1];
				R[3 * r + 1] = c * RE[3 * r + 1] - s * RE[3 * r];
				R[3 * r + 2] = RE[3 * r + 2];
			}
		}
		SAI2B_COL_UNROLL
		for (int r = 0; r < 3; r++) z[i][r] = R[3 * r + 2], o[i][r] = p[r];
		SAI2B_COL_UNROLL
		for (int k = 0; k < COL_MAX_SPHERES; k++) {
			if (k < G.n_spheres && G.link[k] == i) {  // wave-uniform
				SAI2B_COL_UNROLL
				for (int r = 0; r < 3; r++) x[k][r] = p[r] + (R[3 * r] * G.centre[k][0] + R[3 * r + 1] * G.centre[k][1] + R[3 * r + 2] * G.centre[k][2]);
			}
		}
	}
	if (blocks & COL_CENTRES) {
		SAI2B_COL_UNROLL
		for (int k = 0; k < COL_MAX_SPHERES; k++) {
			if (k < G.n_spheres) {
				SAI2B_COL_UNROLL
				for (int a = 0; a < 3; a++) out[(size_t)(G.row[4] + 3 * k + a) * sB] = x[k][a];
			}
		}
	}
	// the sphere a lane's index names: a select over the compile-time k
	auto sphere = [&](int kw, double xw[3], int& lw) {
		xw[0] = xw[1] = xw[2] = 0.0, lw = -1;
		SAI2B_COL_UNROLL
		for (int k = 0; k < COL_MAX_SPHERES; k++) {
			const bool hit = kw == k;
			xw[0] = hit ? x[k][0] : xw[0], xw[1] = hit ? x[k][1] : xw[1], xw[2] = hit ? x[k][2] : xw[2];
			lw = hit ? G.link[k] : lw;
		}
	};
	auto store = [&](int cat, double best, int idx, const double u[3], const double g[DOF]) {
		if (blocks & COL_DISTANCE) out[(size_t)(G.row[0] + cat) * sB] = best;
		if (blocks & COL_INDEX) out[(size_t)(G.row[1] + cat) * sB] = (double)idx;
		if (blocks & COL_NORMAL) {
			SAI2B_COL_UNROLL
			for (int a = 0; a < 3; a++) out[(size_t)(G.row[2] + 3 * cat + a) * sB] = u[a];
		}
		if (blocks & COL_GRADIENT) {
			SAI2B_COL_UNROLL
			for (int m = 0; m < DOF; m++) out[(size_t)(G.row[3] + DOF * cat + m) * sB] = g[m];
		}
	};
	int flags = 0;
	// ---- planes: d = n . (x_k - p0) - r_k, p outer, k inner
	{
		double best = inf;
		int idx = -1;
		SAI2B_COL_UNROLL
		for (int pl = 0; pl < COL_MAX_PLANES; pl++) {
			if (pl < G.n_planes) {
				double w[6];
				SAI2B_COL_UNROLL
				for (int a = 0; a < 6; a++) w[a] = env[(size_t)(COL_PLANE_ROWS * pl + a) * sB];
				SAI2B_COL_UNROLL
				for (int k = 0; k < COL_MAX_SPHERES; k++) {
					if ((G.env_mask >> k) & 1) {
						const double d = (w[3] * (x[k][0] - w[0]) + w[4] * (x[k][1] - w[1]) + w[5] * (x[k][2] - w[2])) - G.radius[k];
						const bool less = d < best;	 // false for a NaN
						best = less ? d : best, idx = less ? 16 * pl + k : idx;
					}
				}
			}
		}
		double u[3] = {0, 0, 0}, g[DOF];
		SAI2B_COL_UNROLL
		for (int m = 0; m < DOF; m++) g[m] = 0.0;
		if (want_normal && idx >= 0) {
			SAI2B_COL_UNROLL
			for (int a = 0; a < 3; a++) u[a] = env[(size_t)(COL_PLANE_ROWS * (idx >> 4) + 3 + a) * sB];
			if (want_gradient) {
				double xw[3];
				int lw;
				sphere(idx & 15, xw, lw);
				col_gradient<DOF>(G, z, o, u, xw, lw, 1.0, g);
			}
		}
		store(COL_PLANE, best, idx, u, g);
		if (best < G.margin[COL_PLANE]) flags |= COL_FLAG_PLANE;
	}
	// ---- obstacles: d = |x_k - c_o| - r_k - r_o, o outer, k inner
	{
		double best = inf;
		int idx = -1;
		const int base = COL_PLANE_ROWS * G.n_planes;
		SAI2B_COL_UNROLL
		for (int ob = 0; ob < COL_MAX_OBSTACLES; ob++) {
			if (ob < G.n_obstacles) {
				double w[4];
				SAI2B_COL_UNROLL
				for (int a = 0; a < 4; a++) w[a] = env[(size_t)(base + COL_OBSTACLE_ROWS * ob + a) * sB];
				SAI2B_COL_UNROLL
				for (int k = 0; k < COL_MAX_SPHERES; k++) {
					if ((G.env_mask >> k) & 1) {
						const double e0 = x[k][0] - w[0], e1 = x[k][1] - w[1], e2 = x[k][2] - w[2];
						const double d = (sqrt(e0 * e0 + e1 * e1 + e2 * e2) - G.radius[k]) - w[3];
						const bool less = d < best;
						best = less ? d : best, idx = less ? 16 * ob + k : idx;
					}
				}
			}
		}
		double u[3] = {0, 0, 0}, g[DOF];
		SAI2B_COL_UNROLL
		for (int m = 0; m < DOF; m++) g[m] = 0.0;
		if (want_normal && idx >= 0) {
			double xw[3];
			int lw;
			sphere(idx & 15, xw, lw);
			double e[3];
			SAI2B_COL_UNROLL
			for (int a = 0; a < 3; a++) e[a] = xw[a] - env[(size_t)(base + COL_OBSTACLE_ROWS * (idx >> 4) + a) * sB];
			const double len = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
			if (len > 0.0) {
				SAI2B_COL_UNROLL
				for (int a = 0; a < 3; a++) u[a] = e[a] / len;
			}
			if (want_gradient) col_gradient<DOF>(G, z, o, u, xw, lw, 1.0, g);
		}
		store(COL_OBSTACLE, best, idx, u, g);
		if (best < G.margin[COL_OBSTACLE]) flags |= COL_FLAG_OBSTACLE;
	}
	// ---- self: d = |x_i - x_j| - r_i - r_j, i outer, j inner, i < j
	{
		double best = inf;
		int idx = -1;
		SAI2B_COL_UNROLL
		for (int i = 0; i < COL_MAX_SPHERES; i++) {
			SAI2B_COL_UNROLL
			for (int j = i + 1; j < COL_MAX_SPHERES; j++) {
				if ((G.pair_mask[i] >> j) & 1) {
					const double e0 = x[i][0] - x[j][0], e1 = x[i][1] - x[j][1], e2 = x[i][2] - x[j][2];
					const double d = (sqrt(e0 * e0 + e1 * e1 + e2 * e2) - G.radius[i]) - G.radius[j];
					const bool less = d < best;
					best = less ? d : best, idx = less ? 16 * i + j : idx;
				}
			}
		}
		double u[3] = {0, 0, 0}, g[DOF];
		SAI2B_COL_UNROLL
		for (int m = 0; m < DOF; m++) g[m] = 0.0;
		if (want_normal && idx >= 0) {
			double xi[3], xj[3];
			int li, lj;
			sphere(idx >> 4, xi, li);
			sphere(idx & 15, xj, lj);
			const double e[3] = {xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2]};
			const double len = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
			if (len > 0.0) {
				SAI2B_COL_UNROLL
				for (int a = 0; a < 3; a++) u[a] = e[a] / len;
			}
			if (want_gradient) {
				col_gradient<DOF>(G, z, o, u, xi, li, 1.0, g);
				col_gradient<DOF>(G, z, o, u, xj, lj, -1.0, g);
			}
		}
		store(COL_SELF, best, idx, u, g);
		if (best < G.margin[COL_SELF]) flags |= COL_FLAG_SELF;
	}
	// a robot whose q is not finite reports that alone
	return finite ? flags : COL_FLAG_NONFINITE;
}

}  // namespace sai2b

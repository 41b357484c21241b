// Test-only harness: the product's trajectory planners (sai2b_otg_group.hpp, sai2b_otg_core.hpp, sai2b_otg3_core.hpp)
// on the device, one input row at a time, for tests/test_gpu_otg_planner.py. Built like sai2b_otg_n*.o (csrc/Makefile):
// -DSAI2B_N=<joints> -include sai2b_dof_rename.h -O3 -std=c++17 -ffp-contract=off. The product never loads this.
//
// A row is n and eight 8-wide vectors, in this order: cp, cv, ca, tp, tv, vmax, amax, jmax (lanes j >= n are padding the
// planners must ignore), plus 6 sample fractions. Per row the harness returns the result code, the duration, per DoF the
// profile's limits / direction / control_signs, its brake duration and its seven phase times, and p, v, a sampled at
// frac * T, T and T + 0.01 (tests/golden/ruckig_record.py: calc3). Acceleration-limited profiles have no limits or
// control signs (-1) and four phases (t0, t1, t2, t6; the rest 0).
//
// Paths: 0 / 1 the sequential planner (otg::calculate / otg3::calculate) on the host, 2 / 3 the group planner
// (otgg::calculate / calculate3, one DoF per lane, 8 lanes per row), 4 / 5 the sequential planner on the device, one
// lane per row (the jerk-limited one is what plan_lane3 runs). Even paths are acceleration-limited, odd ones jerk-limited.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "sai2b_device.hpp"
#if SAI2B_N > 7
#define SAI2B_OTG_MAXD SAI2B_N
#endif
#include "sai2b_otg_core.hpp"
#include "sai2b_otg_group.hpp"
#include "sai2b_otg3_core.hpp"

namespace {
using namespace sai2b;
constexpr int W = 8;		  // row width: lanes of a group
constexpr int NF = 6;		  // sample fractions per row
constexpr int NT = NF + 2;	  // sample times per row
constexpr int MD = otg::MAXD;
static_assert(MD <= W, "a row holds every DoF of the largest generator");

// per-row outputs
struct Out {
	int* res;		// [R]
	double* dur;	// [R]
	int* meta;		// [R][3][W]: limits, direction, control_signs
	double* bdur;	// [R][W]
	double* tph;	// [R][W][7]
	double* pva;	// [R][3][NT][W]
};

__host__ __device__ inline double in_at(const double* in, int r, int k, int j) { return in[((size_t)r * W + k) * W + j]; }
__host__ __device__ inline double sample_time(const double* frac, int r, int k, double T) {
	return k < NF ? frac[(size_t)r * NF + k] * T : k == NF ? T : T + 0.01;
}

// one DoF's outputs (zeros for a failed row or a lane j >= n)
__host__ __device__ inline void put_dof(const Out& o, int r, int j, int lim, int dir, int cs, double bd, const double (&t)[7]) {
	o.meta[((size_t)r * 3 + 0) * W + j] = lim;
	o.meta[((size_t)r * 3 + 1) * W + j] = dir;
	o.meta[((size_t)r * 3 + 2) * W + j] = cs;
	o.bdur[(size_t)r * W + j] = bd;
	for (int i = 0; i < 7; i++) o.tph[((size_t)r * W + j) * 7 + i] = t[i];
}
__host__ __device__ inline void put_sample(const Out& o, int r, int k, int j, double p, double v, double a) {
	o.pva[(((size_t)r * 3 + 0) * NT + k) * W + j] = p;
	o.pva[(((size_t)r * 3 + 1) * NT + k) * W + j] = v;
	o.pva[(((size_t)r * 3 + 2) * NT + k) * W + j] = a;
}
__host__ __device__ inline void put_empty_dof(const Out& o, int r, int j) {
	const double z[7] = {0, 0, 0, 0, 0, 0, 0};
	put_dof(o, r, j, 0, 0, 0, 0.0, z);
	for (int k = 0; k < NT; k++) put_sample(o, r, k, j, 0.0, 0.0, 0.0);
}
__host__ __device__ inline void acc_phases(const otg::Prof& p, double (&t)[7]) {
	t[0] = p.t0, t[1] = p.t1, t[2] = p.t2, t[3] = p.t6, t[4] = t[5] = t[6] = 0.0;
}

// ---- the sequential planners, one row (host, or one device lane) ----
__host__ __device__ void load_input(const double* in, int r, otg::Input& x, double (&vm)[MD], double (&am)[MD], double (&jm)[MD]) {
	for (int d = 0; d < MD; d++) {
		x.cp[d] = in_at(in, r, 0, d), x.cv[d] = in_at(in, r, 1, d), x.ca[d] = in_at(in, r, 2, d);
		x.tp[d] = in_at(in, r, 3, d), x.tv[d] = in_at(in, r, 4, d);
		vm[d] = in_at(in, r, 5, d), am[d] = in_at(in, r, 6, d), jm[d] = in_at(in, r, 7, d);
	}
}
__host__ __device__ void seq_acc(const int* nn, const double* in, const double* frac, const Out& o, int r, otg::Traj& tr) {
	const int n = nn[r];
	otg::Input x;
	double vm[MD], am[MD], jm[MD];
	load_input(in, r, x, vm, am, jm);
	int res = otg::validate(x, n, vm, am) ? otg::calculate(x, n, vm, am, tr) : otg::ERR_INVALID_INPUT;
	o.res[r] = res;
	o.dur[r] = res == otg::WORKING ? tr.duration : 0.0;
	for (int j = 0; j < W; j++) {
		if (res != otg::WORKING || j >= n) {
			put_empty_dof(o, r, j);
			continue;
		}
		const int d = j < MD ? j : 0;
		double t[7];
		acc_phases(tr.prof[d], t);
		put_dof(o, r, j, -1, tr.prof[d].dir, -1, otg::brake_duration(tr.dof[d]), t);
		for (int k = 0; k < NT; k++) {
			double p, v, a;
			otg::at_time(tr.dof[d], tr.prof[d], tr.duration, sample_time(frac, r, k, tr.duration), p, v, a);
			put_sample(o, r, k, j, p, v, a);
		}
	}
}
__host__ __device__ void seq_jerk(const int* nn, const double* in, const double* frac, const Out& o, int r, otg3::Traj& tr) {
	const int n = nn[r];
	otg::Input x;
	double vm[MD], am[MD], jm[MD];
	load_input(in, r, x, vm, am, jm);
	int res = otg3::validate(x, n, vm, am, jm) ? otg3::calculate(x, n, vm, am, jm, tr) : otg::ERR_INVALID_INPUT;
	o.res[r] = res;
	o.dur[r] = res == otg::WORKING ? tr.duration : 0.0;
	for (int j = 0; j < W; j++) {
		if (res != otg::WORKING || j >= n) {
			put_empty_dof(o, r, j);
			continue;
		}
		const otg3::Prof& p = tr.prof[j < MD ? j : 0];
		put_dof(o, r, j, p.limits, p.direction, p.control_signs, p.brake.duration, p.t);
		for (int k = 0; k < NT; k++) {
			double sp, sv, sa;
			otg3::at_time(p, tr.duration, sample_time(frac, r, k, tr.duration), sp, sv, sa);
			put_sample(o, r, k, j, sp, sv, sa);
		}
	}
}

// one lane per row; a small grid strides over the rows so that the per-lane scratch of the planner stays bounded
template <bool JERK> __global__ __launch_bounds__(64) void lane_kernel(int R, const int* nn, const double* in, const double* frac, Out o) {
	for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
		if (JERK) {
			otg3::Traj tr;
			memset(&tr, 0, sizeof(tr));
			seq_jerk(nn, in, frac, o, r, tr);
		} else {
			otg::Traj tr;
			memset(&tr, 0, sizeof(tr));
			seq_acc(nn, in, frac, o, r, tr);
		}
	}
}

// ---- the group planners: group g of the grid takes rows g, g + groups, ... (uniform over the group) ----
template <bool JERK> __global__ __launch_bounds__(64) void group_kernel(int R, const int* nn, const double* in, const double* frac, Out o) {
	const int j = otgg::lane_j();
	const int groups = gridDim.x * (64 / W);
#pragma unroll 1
	for (int r0 = blockIdx.x * (64 / W); r0 < R; r0 += groups) {  // uniform over the wavefront
		const int r = r0 + threadIdx.x / W;
		if (r >= R) continue;  // uniform over the group
		const int n = nn[r];
		const bool active = j < n;
		const double cp = in_at(in, r, 0, j), cv = in_at(in, r, 1, j), ca = in_at(in, r, 2, j), tp = in_at(in, r, 3, j),
					 tv = in_at(in, r, 4, j), vmax = in_at(in, r, 5, j), amax = in_at(in, r, 6, j), jmax = in_at(in, r, 7, j);
		double T = 0.0;
		int res;
		if (JERK) {
			otg3::Prof p;
			memset(&p, 0, sizeof(p));
			res = otgg::calculate3(active, n, cp, cv, ca, tp, tv, vmax, amax, jmax, p, T);
			if (res == otg::WORKING && active) {
				put_dof(o, r, j, p.limits, p.direction, p.control_signs, p.brake.duration, p.t);
				for (int k = 0; k < NT; k++) {
					double sp, sv, sa;
					otg3::at_time(p, T, sample_time(frac, r, k, T), sp, sv, sa);
					put_sample(o, r, k, j, sp, sv, sa);
				}
			}
		} else {
			otg::Dof f;
			otg::Prof p;
			memset(&f, 0, sizeof(f));
			memset(&p, 0, sizeof(p));
			res = otgg::calculate(active, n, cp, cv, ca, tp, tv, vmax, amax, f, p, T);
			if (res == otg::WORKING && active) {
				double t[7];
				acc_phases(p, t);
				put_dof(o, r, j, -1, p.dir, -1, otg::brake_duration(f), t);
				for (int k = 0; k < NT; k++) {
					double sp, sv, sa;
					otg::at_time(f, p, T, sample_time(frac, r, k, T), sp, sv, sa);
					put_sample(o, r, k, j, sp, sv, sa);
				}
			}
		}
		if (res != otg::WORKING || !active) put_empty_dof(o, r, j);
		if (j == 0) o.res[r] = res, o.dur[r] = res == otg::WORKING ? T : 0.0;
	}
}

// ---- the wrapper (OTG_joints: joints_set_goal + update, sai2b_otg_group.hpp) stepped for K ticks, one group per trial.
// The state starts as otg3_test_joints_create + set_limits leave it (tests/cpp/otg_core_test.cpp): reInitialize at x0,
// result FINISHED, epoch 1. Per tick: the goal (gp, gv) if gflag is set, then update(); p, v, a, result, goal_reached
// recorded after it.
template <class LG>
__device__ void stepped_trial(LG& g, int t, int K, double dt, const int* nn, const double* x0, const double* lim, const double* gp,
							  const double* gv, const int* gflag, double* pva, int* rg) {
	const int j = otgg::lane_j();
	const int n = nn[t];
	const bool active = j < n;
	const double vmax = active ? lim[((size_t)t * 3 + 0) * W + j] : 0.0, amax = active ? lim[((size_t)t * 3 + 1) * W + j] : 0.0;
	const double x = active ? x0[(size_t)t * W + j] : 0.0;
	// OTG_joints::reInitialize (joints_reinitialize): setGoal(x0, 0), output = (x0, 0, 0), pass_to_input
	g.target_set = 0;
	otgg::joints_set_goal(g, active, n, x, 0.0);
	g.np = x, g.nv = 0.0, g.na = 0.0;
	if (active) g.in_cp = g.np, g.in_cv = g.nv, g.in_ca = g.na;
	const double epoch = 1.0;
#pragma unroll 1
	for (int k = 0; k < K; k++) {
		const size_t tk = (size_t)t * K + k;
		if (gflag[tk]) otgg::joints_set_goal(g, active, n, active ? gp[tk * W + j] : 0.0, active ? gv[tk * W + j] : 0.0);
		otgg::update(g, false, active, n, dt, vmax, amax, epoch);
		pva[(tk * 3 + 0) * W + j] = active ? g.np : 0.0;
		pva[(tk * 3 + 1) * W + j] = active ? g.nv : 0.0;
		pva[(tk * 3 + 2) * W + j] = active ? g.na : 0.0;
		if (j == 0) rg[tk * 2] = g.result, rg[tk * 2 + 1] = g.goal_reached;
	}
}
template <bool JERK>
__global__ __launch_bounds__(64) void stepped_kernel(int T, int K, double dt, const int* nn, const double* x0, const double* lim,
													 const double* gp, const double* gv, const int* gflag, double* pva, int* rg) {
	const int t = blockIdx.x * (64 / W) + threadIdx.x / W;
	if (t >= T) return;	 // uniform over the group
	if (JERK) {
		otgg::LaneGen3 g;
		memset(&g, 0, sizeof(g));
		g.result = otg::FINISHED;
		g.jmax = otgg::lane_j() < nn[t] ? lim[((size_t)t * 3 + 2) * W + otgg::lane_j()] : 0.0;
		stepped_trial(g, t, K, dt, nn, x0, lim, gp, gv, gflag, pva, rg);
	} else {
		otgg::LaneGen g;
		memset(&g, 0, sizeof(g));
		g.result = otg::FINISHED;
		stepped_trial(g, t, K, dt, nn, x0, lim, gp, gv, gflag, pva, rg);
	}
}

// device buffers of one call, freed on every exit
struct Bufs {
	void* p[16];
	int k = 0;
	~Bufs() {
		for (int i = 0; i < k; i++) (void)hipFree(p[i]);
	}
	template <class T> hipError_t get(T*& d, size_t count, const T* src = nullptr) {
		d = nullptr;
		hipError_t e = hipMalloc((void**)&d, count * sizeof(T) + 1);
		if (e != hipSuccess) return e;
		p[k++] = d;
		return src ? hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice) : hipMemset(d, 0, count * sizeof(T));
	}
};
#define CHK(x)                               \
	do {                                     \
		const hipError_t e_ = (x);           \
		if (e_ != hipSuccess) return (int)e_; \
	} while (0)
}  // namespace

extern "C" {

int otgh_width() { return W; }
int otgh_maxd() { return MD; }

// path: see the file header. Returns 0 or the HIP error code.
int otgh_run(int path, int R, const int* nn, const double* in, const double* frac, int* res, double* dur, int* meta, double* bdur,
			 double* tph, double* pva) {
	if (R <= 0) return 0;
	for (int r = 0; r < R; r++)
		if (nn[r] < 1 || nn[r] > MD) return (int)hipErrorInvalidValue;
	const size_t Rz = (size_t)R;
	if (path == 0 || path == 1) {
		const Out o{res, dur, meta, bdur, tph, pva};
		if (path == 0) {
			otg::Traj* tr = (otg::Traj*)calloc(1, sizeof(otg::Traj));
			for (int r = 0; r < R; r++) memset(tr, 0, sizeof(*tr)), seq_acc(nn, in, frac, o, r, *tr);
			free(tr);
		} else {
			otg3::Traj* tr = (otg3::Traj*)calloc(1, sizeof(otg3::Traj));
			for (int r = 0; r < R; r++) memset(tr, 0, sizeof(*tr)), seq_jerk(nn, in, frac, o, r, *tr);
			free(tr);
		}
		return 0;
	}
	if (path < 2 || path > 5) return (int)hipErrorInvalidValue;
	Bufs b;
	int* d_n;
	double *d_in, *d_frac;
	Out o;
	CHK(b.get(d_n, Rz, nn));
	CHK(b.get(d_in, Rz * W * W, in));
	CHK(b.get(d_frac, Rz * NF, frac));
	CHK(b.get(o.res, Rz));
	CHK(b.get(o.dur, Rz));
	CHK(b.get(o.meta, Rz * 3 * W));
	CHK(b.get(o.bdur, Rz * W));
	CHK(b.get(o.tph, Rz * W * 7));
	CHK(b.get(o.pva, Rz * 3 * NT * W));
	const int rows_per_block = path <= 3 ? 64 / W : 64;
	const int need = (R + rows_per_block - 1) / rows_per_block;
	const int cap = path == 2 ? 4096 : path == 3 ? 1024 : 256;	// the jerk planners' scratch stays bounded (otg3_plan_kernel)
	const dim3 grid(need < cap ? need : cap), block(64);
	if (path == 2) hipLaunchKernelGGL(group_kernel<false>, grid, block, 0, 0, R, d_n, d_in, d_frac, o);
	if (path == 3) hipLaunchKernelGGL(group_kernel<true>, grid, block, 0, 0, R, d_n, d_in, d_frac, o);
	if (path == 4) hipLaunchKernelGGL(lane_kernel<false>, grid, block, 0, 0, R, d_n, d_in, d_frac, o);
	if (path == 5) hipLaunchKernelGGL(lane_kernel<true>, grid, block, 0, 0, R, d_n, d_in, d_frac, o);
	CHK(hipGetLastError());
	CHK(hipDeviceSynchronize());
	CHK(hipMemcpy(res, o.res, Rz * sizeof(int), hipMemcpyDeviceToHost));
	CHK(hipMemcpy(dur, o.dur, Rz * sizeof(double), hipMemcpyDeviceToHost));
	CHK(hipMemcpy(meta, o.meta, Rz * 3 * W * sizeof(int), hipMemcpyDeviceToHost));
	CHK(hipMemcpy(bdur, o.bdur, Rz * W * sizeof(double), hipMemcpyDeviceToHost));
	CHK(hipMemcpy(tph, o.tph, Rz * W * 7 * sizeof(double), hipMemcpyDeviceToHost));
	CHK(hipMemcpy(pva, o.pva, Rz * 3 * NT * W * sizeof(double), hipMemcpyDeviceToHost));
	return 0;
}

// T trials of K ticks: nn [T], x0 [T][W], lim [T][3][W] (vmax, amax, jmax), gp / gv [T][K][W], gflag [T][K];
// out: pva [T][K][3][W], rg [T][K][2] (result, goal_reached). Returns 0 or the HIP error code.
int otgh_stepped(int jerk, int T, int K, double dt, const int* nn, const double* x0, const double* lim, const double* gp, const double* gv,
				 const int* gflag, double* pva, int* rg) {
	if (T <= 0 || K <= 0) return 0;
	for (int t = 0; t < T; t++)
		if (nn[t] < 1 || nn[t] > MD) return (int)hipErrorInvalidValue;
	const size_t Tz = (size_t)T, TK = Tz * (size_t)K;
	Bufs b;
	int *d_n, *d_flag, *d_rg;
	double *d_x0, *d_lim, *d_gp, *d_gv, *d_pva;
	CHK(b.get(d_n, Tz, nn));
	CHK(b.get(d_x0, Tz * W, x0));
	CHK(b.get(d_lim, Tz * 3 * W, lim));
	CHK(b.get(d_gp, TK * W, gp));
	CHK(b.get(d_gv, TK * W, gv));
	CHK(b.get(d_flag, TK, gflag));
	CHK(b.get(d_pva, TK * 3 * W));
	CHK(b.get(d_rg, TK * 2));
	const dim3 grid((T + 64 / W - 1) / (64 / W)), block(64);
	if (jerk)
		hipLaunchKernelGGL(stepped_kernel<true>, grid, block, 0, 0, T, K, dt, d_n, d_x0, d_lim, d_gp, d_gv, d_flag, d_pva, d_rg);
	else
		hipLaunchKernelGGL(stepped_kernel<false>, grid, block, 0, 0, T, K, dt, d_n, d_x0, d_lim, d_gp, d_gv, d_flag, d_pva, d_rg);
	CHK(hipGetLastError());
	CHK(hipDeviceSynchronize());
	CHK(hipMemcpy(pva, d_pva, TK * 3 * W * sizeof(double), hipMemcpyDeviceToHost));
	CHK(hipMemcpy(rg, d_rg, TK * 2 * sizeof(int), hipMemcpyDeviceToHost));
	return 0;
}
}

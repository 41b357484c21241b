// sai2b_host.cpp — host side of the C ABI in include/sai2b.h: configuration helpers (no GPU
// needed), context/buffer management and kernel launches. The numerical work is in
// sai2b_kernels.hip; there is no CPU compute path here — without a GPU sai2b_create() fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "sai2b_launch.h"
#include "sai2b_fast_block.h"
#include "sai2b_snapshot_layout.h"
#include "sai2b_reset_sampler_layout.h"
#include "sai2b_env_sampler_layout.h"
#include "sai2b_model_host.h"
#include "sai2b_baked_panda.h"

using sai2b::DevModel;
using sai2b::rot_from_rpy;
using sai2b::sym3_from6;
using sai2b::DevParams;
using sai2b::DevTask;
using sai2b::TickCall;
using sai2b::TickForm;
using sai2b::WorkList;
constexpr int N = SAI2B_N;  // joints of the robots this build serves (sai2b_params.h)

static thread_local std::string g_error;

// defined once for the whole library by sai2b_dispatch.cpp: the error text of calls that have no context
extern "C" void sai2b_shared_error_set(const char* msg);

struct sai2b_ctx {
	int dof_tag = N;  // FIRST member: sai2b_dispatch.cpp reads it to route a call to the build for this robot size
	int B = 0, T = 0, device = 0;
	bool introspection = false;
	bool models_fresh = false;	// update_task_models() ran for the current state
	bool params_dirty = true;
	bool baked_model = false;  // the ctx model is bit-equal to the compile-time Panda constants
	bool blocking_sync = false;	// SAI2B_BLOCKING_SYNC=1: sai2b_synchronize() blocks without polling first
	// what a tick launches (sai2b_tick_policy.h): the switches of the environment, and the state of the route (the singular mode,
	// the back-off, the pending request for the work list's counts and what the last look said)
	sai2b::RouteSwitches sw;
	sai2b::TickRoute route;
	// work lists (sai2b_launch.h): fb = robots the tick's SVD-free kernel handed to the generic one (counts [4]: with the in-lane
	// singular branch's), rg = the same for the range pass ahead of the trajectory generators, otg = robots that need the trajectory
	// planner this tick (sai2b_otg.hip), tk = the task-level SVD-free kernel's (task_cert_kernel; created on first use).
	// parity: the counter set of the last launch
	WorkList fb, rg, otg, tk;
	// The counts of the tick's work list come back to the host every 8th tick that wants the SVD-free kernel (route.look). By
	// copies: two pinned host words, [0] declined, [1] through the in-lane singular branch, and an event behind them.
	int* fb_seen = nullptr;
	hipEvent_t fb_seen_ev = nullptr;
	// The same counts without copy kernels: three 8-byte words in mapped, coherent pinned memory (fb.report is their device
	// address) that the pass over the work list writes itself (in the self form: a launch of one lane behind the asking tick):
	// [0] = stamp << 32 | declined, [1] = stamp << 32 | in-lane singular, [2] = stamp << 32 | most declined robots of one
	// wavefront. The host asks with a fresh stamp (route.stamp) and, 8 ticks on, waits until all tags carry it. route.by_copy:
	// the pending request went through fb_seen and the event instead (the one-lane generic kernel as the pass does not take
	// the pointer).
	unsigned long long* fb_report = nullptr;
	// sai2b_update_task_models() is deferred: the reference's loop is update -> goal setters -> computeControlTorques,
	// and the fused tick (with the SVD-free kernels in front) does both at once. Any other call in between runs the
	// pending model update first (flush_update), so nothing observable changes.
	bool update_pending = false;
	// The tasks' _current_position / _current_orientation are those of the last torque computation (or
	// re-initialisation), and enabling an OTG starts its generator there (JointTask.cpp:374-376). While
	// the state buffer still holds that state nothing is kept; the first write to it afterwards
	// (set_state, sim_step) saves q here first.
	double* q_pose = nullptr;	// [7][B]
	bool q_is_pose = true;
	// bit t set: task t's goals may have changed since the last OTG update (setters, reinitialize, config
	// updates); goals_exposed: the caller holds the device pointer of some goals buffer, so always assume it
	unsigned goals_dirty = ~0u;
	// Every generator idle (goal reached, goals untouched since): an update is a no-op for every robot, and stays one until the
	// host touches a goal or a generator's configuration — the generator kernels are not launched at all then. Known from the
	// count of non-idle robots otg_kernel leaves behind (read back every 8th tick, consumed 8 ticks later: otg_look) of a tick
	// launched with the goals as they still are (goals_epoch). SAI2B_NO_OTG_IDLE_SKIP=1 switches it off.
	bool otg_all_idle = false, no_otg_idle_skip = false;
	unsigned long long goals_epoch = 0, otg_obs_epoch = 0;
	int* otg_busy_seen = nullptr;  // pinned host word
	hipEvent_t otg_seen_ev = nullptr;
	sai2b::DelayedLook otg_look;  // as route.look: recorded at tick k, consumed at tick k + 8
	bool goals_exposed = false;
	sai2b_robot_model model;
	sai2b_task_config cfg[SAI2B_MAX_TASKS];
	DevParams h_params;
	DevParams* d_params = nullptr;
	hipStream_t stream = nullptr;
	// device-pointer arguments (on_device != 0) are produced / consumed on the caller's stream: ordered against the
	// ctx stream with two events (sai2b_set_caller_stream; default: the legacy default stream)
	hipStream_t caller_stream = nullptr;
	hipEvent_t ev_in = nullptr, ev_out = nullptr;
	double *q = nullptr, *dq = nullptr, *tau = nullptr;
	double* status_buf = nullptr;  // [68][B] scratch of sai2b_get_mft_status
	// per-robot payloads (sai2b_set_link_payload): [0] the controller's rows, [1] the plant's, [10][B] each, created on first use;
	// h_params.payload / plant_payload point at them while that set is in force
	double* payload_rows[2] = {nullptr, nullptr};
	// contact of the plant (sai2b_set_contact): the [9][B] rows, the status rows and the device counter of robots in contact,
	// created on first use; h_params.contact points at the rows while a contact is in force
	double* contact_rows = nullptr;
	sai2b_contact_config contact_cfg = {};
	// joint dynamics of the plant (sai2b_set_joint_dynamics): the [6][dof][B] rows, the [3][dof][B] status rows and the two device
	// counters, created on first use; joint_on: sai2b_sim_step launches sim_joint_kernel with `joint` as its argument
	bool joint_on = false;
	sai2b_joint_dynamics_config joint_cfg = {};
	sai2b::JointParams joint;
	double *joint_rows = nullptr, *joint_status = nullptr;
	int* joint_counts = nullptr;
	// external wrench on a link of the plant (sai2b_set_external_wrench): the [7][B] rows, the [6 + dof][B] status rows and the device
	// counter of robots pushed, created on first use; wrench_on: sai2b_sim_step launches the wrench forms with `wrench` as their argument
	bool wrench_on = false;
	sai2b_external_wrench_config wrench_cfg = {};
	sai2b::WrenchParams wrench;
	double *wrench_rows = nullptr, *wrench_status = nullptr;
	int* wrench_count = nullptr;
	// actuator and force-sensor models (sai2b_set_hardware), created on first use: the [1 + 3 dof][B] actuator rows, the [13][B]
	// sensor rows, the torque history (room for the deepest, [SAI2B_MAX_ACTUATION_DELAY + 1][dof][B]; hw_cfg.max_delay + 1 slots
	// are in use), the filter states f, g [dof + 6][B], the applied torques [dof][B] and the clocks (period, episode) [2][B].
	// hw_on: sai2b_sim_step launches actuate_kernel ahead of the simulation kernel and, when due, sense_kernel behind it
	bool hw_on = false;
	sai2b_hardware_config hw_cfg = {};
	double *hw_act = nullptr, *hw_sensor = nullptr, *hw_history = nullptr, *hw_filter = nullptr, *hw_applied = nullptr;
	int* hw_clock = nullptr;
	// joint sensors (sai2b_set_joint_sensor), created on first use: the [1 + 5 dof][B] rows, the measured pair, the previous position
	// reading and the velocity filter's state [dof][B] each, the history of readings (room for the deepest,
	// [SAI2B_MAX_ACTUATION_DELAY + 1][2 dof][B]; js_cfg.max_delay + 1 slots are in use), the clocks (next reading, episode) [2][B] and
	// d_params_meas, the device copy of h_params whose q, dq are the measured pair. js_on: the controller-side launches take
	// d_params_meas (ctrl_params), sai2b_sim_step launches joint_sense_kernel last, and while q_is_pose holds the cached pose
	// is the measured q (ctrl_q)
	bool js_on = false;
	sai2b_joint_sensor_config js_cfg = {};
	double *js_rows = nullptr, *js_qm = nullptr, *js_dqm = nullptr, *js_prev = nullptr, *js_filter = nullptr, *js_history = nullptr;
	int* js_clock = nullptr;
	DevParams* d_params_meas = nullptr;
	// collision proximity (sai2b_set_collision), created on first use: the environment rows (room for the largest,
	// [6 * 2 + 4 * 4][B]), the five device counters of the last query and, behind them, the counter of the last sai2b_end_episodes
	// (col_counts is allocated by either), col_out / col_flags: staging of a query with host arguments (col_out_rows: rows col_out
	// has room for), end_done / end_extra: staging of sai2b_end_episodes with host arguments. col_on: the configuration is in
	// force; nothing else in the context reads it
	bool col_on = false;
	sai2b_collision_config col_cfg = {};
	sai2b::ColParams col;
	int col_rows = 0, col_env_rows = 0, col_out_rows = 0;
	double *col_env = nullptr, *col_out = nullptr;
	unsigned char *col_flags = nullptr, *end_done = nullptr, *end_extra = nullptr;
	int* col_counts = nullptr;
	// inverse kinematics (sai2b_set_ik): the configuration in force, the four device counters of the last solve, and the staging
	// of a solve with host arguments (ik_rows: goal 12 + N, seed N, q_out N, status 5 rows; ik_bytes: mask and flags), created
	// on first use. Nothing else in the context reads any of it
	bool ik_on = false;
	sai2b_ik_config ik_cfg = {};
	int* ik_counts = nullptr;
	double* ik_rows = nullptr;
	unsigned char* ik_bytes = nullptr;
	// whole-arm contact of the plant (sai2b_set_body_contact), created on first use: the [3][B] rows, the [9 + dof][B] status rows
	// and the four device counters. body_on: sai2b_sim_step launches sim_body_kernel; its geometry is taken from `col` at every
	// step, so it follows the collision configuration (which must be in force: sai2b_clear_collision clears this too)
	bool body_on = false;
	sai2b_body_contact_config body_cfg = {};
	double *body_rows = nullptr, *body_status = nullptr;
	int* body_counts = nullptr;
	double* sim_tau = nullptr;	// staging for host torques / bias read-back of the simulation harness
	// observations and episode-end flags (sai2b_set_observation): the configuration in force and what observe_kernel takes
	// from it, the per-robot episode counters and the device counters of the last observe, created on first use; obs_out /
	// obs_done stage the results of a call with host arguments (obs_out_rows: rows obs_out has room for)
	bool obs_on = false;
	sai2b_observation_config obs_cfg = {};
	sai2b::ObsParams obs;
	int obs_rows = 0, obs_out_rows = 0;
	int *obs_steps = nullptr, *obs_counts = nullptr;
	double* obs_out = nullptr;
	unsigned char* obs_done = nullptr;
	// rewards and episode returns (sai2b_set_reward): the configuration in force and what observe_reward_kernel takes from it, the
	// per-robot accumulators (SAI2B_BUF_REWARD_STATE / _EPISODE) and the device counters of the last call, created on first use;
	// rew_out stages reward [B] and terms [rew_rows][B] of a call with host arguments
	bool rew_on = false;
	sai2b_reward_config rew_cfg = {};
	sai2b::RewParams rew;
	int rew_rows = 0;
	double *rew_state = nullptr, *rew_out = nullptr;
	int *rew_episode = nullptr, *rew_counts = nullptr;	// rew_counts: obs_counts + OBS_COUNTS
	// actions (sai2b_set_action): the configuration in force and what action_kernel takes from it, the device counters of the
	// last apply, created on first use; act_in / act_mask stage the inputs of a call with host arguments (act_in_rows: rows
	// act_in has room for)
	bool act_on = false;
	sai2b_action_config act_cfg = {};
	sai2b::ActParams act;
	int act_rows = 0, act_in_rows = 0;
	int* act_counts = nullptr;
	double* act_in = nullptr;
	unsigned char* act_mask = nullptr;
	// episode sampler (sai2b_set_reset_sampler): the configuration in force and its row layout, the per-robot rows (room for
	// rs_rows_cap rows), the episode counters and the tries of the last reset [2][B] and the device counters of the last call,
	// created on first use
	bool rs_on = false;
	sai2b_reset_sampler_config rs_cfg = {};
	sai2b::RsLayout rs_lay;
	double* rs_rows = nullptr;
	int rs_rows_cap = 0;
	int *rs_state = nullptr, *rs_counts = nullptr;
	// environment sampler (sai2b_set_env_sampler): the configuration in force and its sample-row layout (es_lay stays that of the
	// last set after a clear: the snapshot layout reads it), the nominal rows (sai2b::EnvNominal), the sample rows (room for
	// es_sample_cap rows), the draw counters [B] and the device counters of the last call, created on first use
	bool es_on = false;
	sai2b_env_sampler_config es_cfg = {};
	sai2b::EnvLayout es_lay;
	double *es_nominal = nullptr, *es_sample = nullptr;
	int es_sample_cap = 0;
	int *es_counter = nullptr, *es_counts = nullptr;
	// sai2b_reinitialize_robots / sai2b_reset_robots with host arguments: the [B]-byte mask and the [2 * dof][B] q, dq rows are
	// staged here, created on first use
	unsigned char* reset_mask = nullptr;
	double* reset_rows = nullptr;
	// snapshot banks (sai2b_snapshot_save / _load), created with the first bank: the four device words the kernel counts in, the
	// three mapped host words the counts of a call arrive in (tagged with snap_stamp; snap_report_dev is their device address)
	// and the staging of a host slot array (a host mask goes through reset_mask)
	int* snap_counts = nullptr;
	unsigned long long *snap_report = nullptr, *snap_report_dev = nullptr;
	unsigned snap_stamp = 0;
	int* snap_slot = nullptr;
	// task-level calls (TemplateTask.h:42-88): per task the caller's N_prec, the task's N and N * N_prec of the
	// last sai2b_task_update_model, its torques and a staging copy of a host tau_prec; created on first use
	int last_call_task = 0;	  // the last launch sequence was a task-level call: 1 = task_cert_kernel + work list, 2 = the generic task kernel alone
	struct TaskIO {
		double *Nprec = nullptr, *N = nullptr, *Ntot = nullptr, *tau = nullptr, *tau_prec = nullptr;
		bool nprec_given = false;  // false: identity (the value a task is constructed with)
		bool model_fresh = false;  // sai2b_task_update_model ran for the current state
		bool standalone = false;   // the task is being driven through the task-level calls
	} tio[SAI2B_MAX_TASKS];
	std::vector<void*> allocs;
	long long launches = 0, ticks = 0;
	std::string error;
};

static int flush_update(sai2b_ctx* ctx);  // runs a deferred sai2b_update_task_models() now

// the controller's view of the state (include/sai2b.h "joint sensors"): the measured pair with a joint sensor, else the truth
static const DevParams* ctrl_params(const sai2b_ctx* ctx) { return ctx->js_on ? ctx->d_params_meas : ctx->d_params; }
static double* ctrl_q(const sai2b_ctx* ctx) { return ctx->js_on ? ctx->js_qm : ctx->q; }
static double* ctrl_dq(const sai2b_ctx* ctx) { return ctx->js_on ? ctx->js_dqm : ctx->dq; }

static int set_error(sai2b_ctx* ctx, int code, const std::string& msg) {
	g_error = msg;
	sai2b_shared_error_set(msg.c_str());
	if (ctx) ctx->error = msg;
	return code;
}
#define HIP_TRY(ctx, expr)                                                                         \
	do {                                                                                           \
		hipError_t e_ = (expr);                                                                    \
		if (e_ != hipSuccess)                                                                      \
			return set_error(ctx, SAI2B_RUNTIME_ERROR, std::string(#expr) + ": " + hipGetErrorString(e_)); \
	} while (0)

// ------------------------------------------------------------------------------------------------
// small host-side linear algebra for the configuration helpers
// ------------------------------------------------------------------------------------------------
// cyclic Jacobi eigen-decomposition of a symmetric n x n matrix (n <= 7): A = V diag(w) V^T
static void sym_eig(int n, const double* A_in, double* w, double* V) {
	double A[49];
	std::memcpy(A, A_in, sizeof(double) * n * n);
	for (int i = 0; i < n * n; i++) V[i] = 0;
	for (int i = 0; i < n; i++) V[i * n + i] = 1;
	for (int sweep = 0; sweep < 64; sweep++) {
		double off = 0;
		for (int i = 0; i < n; i++)
			for (int j = i + 1; j < n; j++) off += A[i * n + j] * A[i * n + j];
		if (off < 1e-300) break;
		for (int p = 0; p < n; p++)
			for (int q = p + 1; q < n; q++) {
				const double apq = A[p * n + q];
				if (std::fabs(apq) < 1e-300) continue;
				const double theta = (A[q * n + q] - A[p * n + p]) / (2 * apq);
				const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
				const double c = 1 / std::sqrt(t * t + 1), s = t * c;
				for (int k = 0; k < n; k++) {
					const double akp = A[k * n + p], akq = A[k * n + q];
					A[k * n + p] = c * akp - s * akq;
					A[k * n + q] = s * akp + c * akq;
				}
				for (int k = 0; k < n; k++) {
					const double apk = A[p * n + k], aqk = A[q * n + k];
					A[p * n + k] = c * apk - s * aqk;
					A[q * n + k] = s * apk + c * aqk;
				}
				for (int k = 0; k < n; k++) {
					const double vkp = V[k * n + p], vkq = V[k * n + q];
					V[k * n + p] = c * vkp - s * vkq;
					V[k * n + q] = s * vkp + c * vkq;
				}
			}
	}
	for (int i = 0; i < n; i++) w[i] = A[i * n + i];
}
// Orthogonal projector onto the range of the 3 x nd matrix whose columns are the given directions,
// with the rank rule of Sai2Model::matrixRangeBasis (sigma_i / sigma_0 >= 1e-3, zero if
// sigma_0 < 1e-3). Returns the rank. (MotionForceTask.cpp:55-87,146-152)
static int direction_projector(int nd, const double* dirs, double* P) {
	for (int i = 0; i < 9; i++) P[i] = 0;
	if (nd <= 0) return 0;
	double G[9] = {0};
	for (int d = 0; d < nd; d++)
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) G[3 * i + j] += dirs[3 * d + i] * dirs[3 * d + j];
	double w[3], V[9];
	sym_eig(3, G, w, V);
	double s[3], s0 = 0;
	for (int i = 0; i < 3; i++) {
		s[i] = std::sqrt(std::max(w[i], 0.0));
		s0 = std::max(s0, s[i]);
	}
	if (s0 < 1e-3) return 0;
	int rank = 0;
	const int p = std::min(3, nd);
	// keep at most min(3, nd) directions, those above the relative tolerance
	int order[3] = {0, 1, 2};
	std::sort(order, order + 3, [&](int a, int b) { return s[a] > s[b]; });
	for (int k = 0; k < p; k++)
		if (k == 0 || s[order[k]] / s0 >= 1e-3) rank++;
	if (rank == 3) {
		P[0] = P[4] = P[8] = 1;
		return 3;
	}
	for (int k = 0; k < rank; k++) {
		const int c = order[k];
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) P[3 * i + j] += V[3 * i + c] * V[3 * j + c];
	}
	return rank;
}
// rank of a k x 7 matrix by Gaussian elimination with full pivoting (Eigen::FullPivLU::rank(),
// JointTask.cpp:34-35)
static int full_pivot_rank(int rows, int cols, const double* A_in) {
	std::vector<double> A(A_in, A_in + rows * cols);
	int rank = 0;
	double maxpiv = 0;
	const int p = std::min(rows, cols);
	std::vector<int> rused(rows, 0), cused(cols, 0);
	for (int step = 0; step < p; step++) {
		int pr = -1, pc = -1;
		double best = 0;
		for (int r = 0; r < rows; r++)
			if (!rused[r])
				for (int c = 0; c < cols; c++)
					if (!cused[c] && std::fabs(A[r * cols + c]) > best) {
						best = std::fabs(A[r * cols + c]);
						pr = r;
						pc = c;
					}
		if (pr < 0) break;
		if (step == 0) maxpiv = best;
		if (best <= maxpiv * 2.220446049250313e-16 * p) break;
		rank++;
		rused[pr] = cused[pc] = 1;
		for (int r = 0; r < rows; r++) {
			if (rused[r]) continue;
			const double f = A[r * cols + pc] / A[pr * cols + pc];
			for (int c = 0; c < cols; c++) A[r * cols + c] -= f * A[pr * cols + c];
		}
	}
	return rank;
}

// ------------------------------------------------------------------------------------------------
// configuration helpers (host only)
// ------------------------------------------------------------------------------------------------

extern "C" int sai2b_model_merge_fixed_body(sai2b_robot_model* md, int link, const double xyz[3], const double rpy[3],
											double mass, const double com[3], const double inertia[6]) {
	if (!md || link < 0 || link >= N || !xyz || !rpy || !com || !inertia)
		return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_model_merge_fixed_body: bad arguments");
	sai2b::host_merge_fixed_body(md, link, xyz, rpy, mass, com, inertia);
	return SAI2B_OK;
}

extern "C" int sai2b_panda_model(sai2b_robot_model* md) {
	if (!md) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_panda_model: null");
	sai2b::host_panda_model(md);
	return SAI2B_OK;
}

static void singularity_defaults(sai2b_task_config* c) {
	c->s_min = 6e-3, c->s_max = 6e-2;  // MotionForceTask.cpp:197
	c->s_abs_tol = 1e-3;			   // SingularityHandler.cpp:11-19
	c->type_1_tol = 0.5;
	c->type_2_torque_ratio = 1e-2;
	c->type_2_angle_threshold = 5 * M_PI / 180;
	c->perturb_step_size = 5;
	c->sh_buffer_size = SAI2B_SH_HISTORY;
	c->kp_type_1 = 50, c->kv_type_1 = 14, c->kv_type_2 = 5;
	c->enforce_type_1_strategy = 0;	 // SingularityHandler.cpp:63-64
	c->enforce_handling_strategy = 1;
}

extern "C" int sai2b_default_joint_task(sai2b_task_config* c, const char* name, int task_dof, const double* selection) {
	if (!c) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_joint_task: null config");
	std::memset(c, 0, sizeof(*c));
	c->type = SAI2B_JOINT_TASK;
	std::snprintf(c->name, sizeof(c->name), "%s", name ? name : "joint_task");
	c->loop_timestep = 0.001;
	c->dynamic_decoupling_type = SAI2B_BOUNDED_INERTIA_ESTIMATES;
	c->bie_threshold = 0.1;
	if (!selection) {
		c->task_dof = N;
		for (int i = 0; i < N; i++) c->joint_selection[i * N + i] = 1;
	} else {
		if (task_dof < 1 || task_dof > N)
			return set_error(nullptr, SAI2B_INVALID_ARGUMENT,
							 "joint selection matrix size not consistent with robot dof in JointTask constructor\n");
		if (full_pivot_rank(task_dof, N, selection) != task_dof)
			return set_error(nullptr, SAI2B_INVALID_ARGUMENT,
							 "joint selection matrix is not full rank in JointTask constructor\n");
		c->task_dof = task_dof;
		std::memcpy(c->joint_selection, selection, sizeof(double) * task_dof * N);
	}
	for (int i = 0; i < N; i++) {
		c->kp[i] = 50.0, c->kv[i] = 14.0, c->ki[i] = 0.0;  // JointTask.h:32-34
		c->saturation_velocity[i] = M_PI / 3.0;				 // JointTask.h:44
		c->otg_max_velocity[i] = M_PI / 3.0;				 // JointTask.h:40
		c->otg_max_acceleration[i] = 2.0 * M_PI;			 // JointTask.h:41
	}
	c->use_internal_otg = 1;  // JointTask.h:38-39: on, acceleration-limited
	c->internal_otg_jerk_limited = 0;
	for (int i = 0; i < SAI2B_MAX_DOF; i++) c->otg_max_jerk[i] = 10.0 * M_PI;  // JointTask.h:42
	c->robot_dof = N;
	return SAI2B_OK;
}

extern "C" int sai2b_default_motion_force_task(sai2b_task_config* c, const char* name, int link,
											   const double frame_pos[3], const double* frame_rot, int n_trans,
											   const double* dirs_trans, int n_rot, const double* dirs_rot) {
	if (!c) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_motion_force_task: null config");
	std::memset(c, 0, sizeof(*c));
	c->type = SAI2B_MOTION_FORCE_TASK;
	const bool partial = !(n_trans < 0 && n_rot < 0);
	std::snprintf(c->name, sizeof(c->name), "%s", name ? name : (partial ? "partial_motion_force_task" : "motion_force_task"));
	c->loop_timestep = 0.001;
	if (link < 0 || link >= N) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "MotionForceTask: link index out of range");
	c->link = link;
	for (int i = 0; i < 3; i++) c->frame_pos[i] = frame_pos ? frame_pos[i] : 0.0;
	for (int i = 0; i < 9; i++) c->frame_rot[i] = frame_rot ? frame_rot[i] : (i % 4 == 0 ? 1.0 : 0.0);
	const char* empty_msg =
		"controlled_directions_translation and controlled_directions_rotation cannot both be empty in "
		"MotionForceTask::MotionForceTask\n";
	if (!partial) {
		for (int i = 0; i < 6; i++) c->partial_projection[i * 6 + i] = 1;
		c->pos_range = c->ori_range = 3;
	} else {
		if (std::max(n_trans, 0) + std::max(n_rot, 0) == 0) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, empty_msg);
		if ((n_trans > 0 && !dirs_trans) || (n_rot > 0 && !dirs_rot))
			return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "MotionForceTask: null direction array");
		double Pp[9], Po[9];
		c->pos_range = direction_projector(n_trans, dirs_trans, Pp);
		c->ori_range = direction_projector(n_rot, dirs_rot, Po);
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) {
				c->partial_projection[i * 6 + j] = Pp[3 * i + j];
				c->partial_projection[(3 + i) * 6 + 3 + j] = Po[3 * i + j];
			}
		if (c->pos_range + c->ori_range == 0) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, empty_msg);
	}
	c->dynamic_decoupling_type = SAI2B_BOUNDED_INERTIA_ESTIMATES;
	c->bie_threshold = 0.1;
	for (int i = 0; i < 3; i++) {  // MotionForceTask.h:44-55
		c->kp_pos[i] = 100.0, c->kv_pos[i] = 20.0, c->ki_pos[i] = 0.0;
		c->kp_ori[i] = 200.0, c->kv_ori[i] = 28.3, c->ki_ori[i] = 0.0;
		c->kp_force[i] = 0.7, c->kv_force[i] = 10.0, c->ki_force[i] = 1.3;
		c->kp_moment[i] = 0.7, c->kv_moment[i] = 10.0, c->ki_moment[i] = 1.3;
	}
	c->kff_force = c->kff_moment = 0.95;
	c->max_force_feedback = 20.0, c->max_moment_feedback = 10.0;
	c->force_axis[2] = c->moment_axis[2] = 1.0;
	c->linear_saturation_velocity = 0.3, c->angular_saturation_velocity = M_PI / 3;
	c->sensor_rot[0] = c->sensor_rot[4] = c->sensor_rot[8] = 1.0;
	singularity_defaults(c);
	c->use_internal_otg = 1;  // MotionForceTask.h:67-72: on, acceleration-limited
	c->internal_otg_jerk_limited = 0;
	c->otg_max_linear_jerk = 10.0, c->otg_max_angular_jerk = 10.0 * M_PI;  // MotionForceTask.h:73-74
	c->otg_max_linear_velocity = 0.3, c->otg_max_linear_acceleration = 2.0;
	c->otg_max_angular_velocity = M_PI / 3, c->otg_max_angular_acceleration = 2.0 * M_PI;
	c->robot_dof = N;
	return SAI2B_OK;
}

extern "C" int sai2b_validate_tasks(const sai2b_task_config* tasks, int n_tasks, char* msg, int msg_len) {
	std::string err;
	if (!tasks || n_tasks <= 0)
		err = "RobotController must have at least one task";
	else if (n_tasks > SAI2B_MAX_TASKS)
		err = "too many tasks for this build (SAI2B_MAX_TASKS)";
	bool closed = false;
	for (int i = 0; err.empty() && i < n_tasks; i++) {
		const sai2b_task_config& t = tasks[i];
		if (t.type != SAI2B_JOINT_TASK && t.type != SAI2B_MOTION_FORCE_TASK)
			err = "task type must be JOINT_TASK or MOTION_FORCE_TASK";
		else if ((t.robot_dof ? t.robot_dof : SAI2B_DOF) != N)
			err = "task was configured for a robot with another number of joints (sai2b_task_config.robot_dof)";
		else if (t.loop_timestep != tasks[0].loop_timestep)
			err = "All tasks must have the same loop timestep in RobotController";
		for (int j = 0; err.empty() && j < i; j++)
			if (std::strncmp(t.name, tasks[j].name, sizeof(t.name)) == 0) err = "Tasks in RobotController must have unique names";
		if (err.empty() && closed)
			err = std::string("task [") + t.name +
				  "] cannot be added to the controller because it is in the nullspace of a full joint task";
		if (err.empty() && t.type == SAI2B_JOINT_TASK) {
			if (t.task_dof < 1 || t.task_dof > N)
				err = "joint selection matrix size not consistent with robot dof in JointTask constructor\n";
			else if (full_pivot_rank(t.task_dof, N, t.joint_selection) != t.task_dof)
				err = "joint selection matrix is not full rank in JointTask constructor\n";
			else if (t.task_dof == N)
				closed = true;	// isFullJointTask (RobotController.cpp:44-49)
			for (int k = 0; err.empty() && k < t.task_dof && !t.unsafe_motion_gains; k++)	// (setGainsUnsafe: JointTask.cpp:136-156)
				if (t.kp[k] < 0 || t.kv[k] < 0 || t.ki[k] < 0) err = "gains must be positive or zero in JointTask::setGains\n";
		}
		if (err.empty() && t.type == SAI2B_MOTION_FORCE_TASK) {
			if (t.link < 0 || t.link >= N) err = "MotionForceTask: link index out of range";
			if (t.force_space_dimension < 0 || t.force_space_dimension > 3)
				err = "Force space dimension should be between 0 and 3 in MotionForceTask::parametrizeForceMotionSpaces\n";
			if (t.moment_space_dimension < 0 || t.moment_space_dimension > 3)
				err = "Moment space dimension should be between 0 and 3 in MotionForceTask::parametrizeMomentRotMotionSpaces\n";
			if (t.sh_buffer_size < 1 || t.sh_buffer_size > SAI2B_SH_HISTORY) err = "singularity history size must be in [1, 200]";
			for (int k = 0; err.empty() && k < 3 && !t.unsafe_motion_gains; k++)
				if (t.kp_pos[k] < 0 || t.kv_pos[k] < 0 || t.ki_pos[k] < 0 || t.kp_ori[k] < 0 || t.kv_ori[k] < 0 || t.ki_ori[k] < 0)
					err = "all gains should be positive or zero in MotionForceTask::setPosControlGains\n";
			// the single axis of a 1- or 2-dimensional force / moment space must be a direction (MotionForceTask.cpp:840-848,868-876)
			auto axis_norm = [](const double* a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
			if (err.empty() && (t.force_space_dimension == 1 || t.force_space_dimension == 2) && !(axis_norm(t.force_axis) >= 1e-2))
				err = "Force or motion axis should be a non singular vector in MotionForceTask::parametrizeForceMotionSpaces\n";
			if (err.empty() && (t.moment_space_dimension == 1 || t.moment_space_dimension == 2) && !(axis_norm(t.moment_axis) >= 1e-2))
				err = "Moment or rot motion axis should be a non singular vector in MotionForceTask::parametrizeMomentRotMotionSpaces\n";
			// pos_range / ori_range are the ranks of the two diagonal blocks of the projection (MotionForceTask.cpp:146-152)
			if (err.empty()) {
				double w[6], V[36];
				sym_eig(6, t.partial_projection, w, V);
				int rank = 0;
				bool projector = true;
				for (int k = 0; k < 6; k++) {
					if (std::fabs(w[k] - 1.0) < 1e-9)
						rank++;
					else if (std::fabs(w[k]) > 1e-9)
						projector = false;
				}
				if (!projector || rank != t.pos_range + t.ori_range || t.pos_range < 0 || t.pos_range > 3 || t.ori_range < 0 || t.ori_range > 3 ||
					rank == 0)
					err = "MotionForceTask: partial_projection must be an orthogonal projector of rank pos_range + ori_range >= 1";
			}
		}
		if (err.empty() && (t.singular_vector_sign < SAI2B_SV_SIGN_V_MAX_POSITIVE || t.singular_vector_sign > SAI2B_SV_SIGN_BOTH))
			err = "singular_vector_sign must be one of enum sai2b_singular_vector_sign";
		if (err.empty() && (t.dynamic_decoupling_type < SAI2B_FULL_DYNAMIC_DECOUPLING || t.dynamic_decoupling_type > SAI2B_IMPEDANCE))
			err = "dynamic_decoupling_type must be FULL_DYNAMIC_DECOUPLING, BOUNDED_INERTIA_ESTIMATES or IMPEDANCE";
		if (err.empty() && t.use_internal_otg && t.internal_otg_jerk_limited) {	 // setMaxJerk (OTG_joints.cpp:73-86, OTG_6dof_cartesian.cpp:126-136)
			if (t.type == SAI2B_JOINT_TASK) {
				for (int k = 0; err.empty() && k < t.task_dof; k++)
					if (!(t.otg_max_jerk[k] > 0) || std::isinf(t.otg_max_jerk[k]))
						err = "max jerk cannot be 0 or negative in any directions in OTG_joints::setMaxJerk\n";
			} else if (!(t.otg_max_linear_jerk > 0) || !(t.otg_max_angular_jerk > 0) || std::isinf(t.otg_max_linear_jerk) ||
					   std::isinf(t.otg_max_angular_jerk)) {
				err = "max jerk set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxJerk\n";
			}
		}
		if (err.empty() && t.use_internal_otg) {
			if (t.type == SAI2B_JOINT_TASK) {
				for (int k = 0; err.empty() && k < t.task_dof; k++) {
					if (!(t.otg_max_velocity[k] > 0))
						err = "max velocity cannot be 0 or negative in any directions in OTG_joints::setMaxVelocity\n";
					else if (!(t.otg_max_acceleration[k] > 0))
						err = "max acceleration cannot be 0 or negative in any directions in OTG_joints::setMaxAcceleration\n";
				}
			} else if (!(t.otg_max_linear_velocity > 0) || !(t.otg_max_angular_velocity > 0)) {
				err = "max velocity set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxLinearVelocity\n";
			} else if (!(t.otg_max_linear_acceleration > 0) || !(t.otg_max_angular_acceleration > 0)) {
				err = "max acceleration set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxLinearAcceleration\n";
			}
		}
		if (err.empty() && t.use_velocity_saturation) {
			if (t.type == SAI2B_MOTION_FORCE_TASK && (t.linear_saturation_velocity <= 0 || t.angular_saturation_velocity <= 0))
				err = "Velocity saturation values should be strictly positive or zero in MotionForceTask::enableVelocitySaturation\n";
			if (t.type == SAI2B_JOINT_TASK)
				for (int k = 0; k < t.task_dof; k++)
					if (t.saturation_velocity[k] <= 0) err = "saturation velocity must be positive in JointTask::enableVelocitySaturation\n";
		}
	}
	// implementation restriction: one shared bounded-inertia estimate per tick
	double thr = -1;
	for (int i = 0; err.empty() && i < n_tasks; i++)
		if (tasks[i].dynamic_decoupling_type == SAI2B_BOUNDED_INERTIA_ESTIMATES) {
			if (thr >= 0 && tasks[i].bie_threshold != thr)
				err = "tasks using BOUNDED_INERTIA_ESTIMATES must share one threshold in this build";
			thr = tasks[i].bie_threshold;
		}
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
// the reference's setters keep the single axis normalised (MotionForceTask.cpp:840-848,868-876): C callers need not
static void normalise_axes(sai2b_task_config& c) {
	if (c.type != SAI2B_MOTION_FORCE_TASK) return;
	for (double* a : {c.force_axis, c.moment_axis}) {
		const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
		if (n >= 1e-2)
			for (int k = 0; k < 3; k++) a[k] /= n;
	}
}

static void fill_dev_task(const sai2b_task_config& c, DevTask& d) {
	d.type = c.type;
	d.decoupling = c.dynamic_decoupling_type;
	d.bie_threshold = c.bie_threshold;
	d.dt = c.loop_timestep;
	d.k0 = c.type == SAI2B_JOINT_TASK ? c.task_dof : 0;
	for (int i = 0; i < N * N; i++) d.S[i] = 0;
	bool ident = (d.k0 == N);
	for (int i = 0; i < d.k0; i++)
		for (int j = 0; j < N; j++) {
			d.S[i * N + j] = c.joint_selection[i * N + j];
			if (d.S[i * N + j] != (i == j ? 1.0 : 0.0)) ident = false;
		}
	d.full_selection = ident ? 1 : 0;
	for (int i = 0; i < N; i++) d.kp[i] = c.kp[i], d.kv[i] = c.kv[i], d.ki[i] = c.ki[i], d.vsat[i] = c.saturation_velocity[i];
	d.use_vsat = c.use_velocity_saturation;
	d.link = c.link;
	std::memcpy(d.frame_pos, c.frame_pos, sizeof(d.frame_pos));
	std::memcpy(d.frame_rot, c.frame_rot, sizeof(d.frame_rot));
	{
		// is the compliant frame's linear part a rotation (orthonormal, det +1)? Then a pose of the control frame is its
		// position and two columns of its orientation (cert::singular_part keeps it that way); anything else the
		// reference would accept too, and it is carried as the nine numbers it is
		const double* R = c.frame_rot;
		double worst = 0;
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) {
				double g = 0;
				for (int k = 0; k < 3; k++) g += R[3 * k + i] * R[3 * k + j];
				worst = std::fmax(worst, std::fabs(g - (i == j ? 1.0 : 0.0)));
			}
		const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
		d.frame_rigid = (worst < 1e-12 && det > 0) ? 1 : 0;
	}
	std::memcpy(d.P, c.partial_projection, sizeof(d.P));
	bool pid = true;
	for (int i = 0; i < 36; i++)
		if (c.partial_projection[i] != ((i % 7 == 0) ? 1.0 : 0.0)) pid = false;
	d.full_projection = pid ? 1 : 0;
	d.rank = c.pos_range + c.ori_range;
	{
		int lead = 0;
		bool diag01 = true;
		for (int i = 0; i < 6; i++)
			for (int j = 0; j < 6; j++) {
				const double v = c.partial_projection[i * 6 + j];
				if (i != j && v != 0.0) diag01 = false;
				if (i == j && v != 0.0 && v != 1.0) diag01 = false;
			}
		while (lead < 6 && c.partial_projection[lead * 7] == 1.0) lead++;
		for (int i = lead; i < 6; i++)
			if (c.partial_projection[i * 7] != 0.0) diag01 = false;
		d.p_lead = diag01 ? lead : 6;
	}
	{  // basis of range(P): eigenvectors of the projector with eigenvalue 1
		double w[6], V[36];
		sym_eig(6, c.partial_projection, w, V);
		for (int i = 0; i < 36; i++) d.PU[i] = 0;
		int col = 0;
		for (int j = 0; j < 6 && col < d.rank; j++)
			if (w[j] > 0.5) {
				for (int i = 0; i < 6; i++) d.PU[i * 6 + col] = V[i * 6 + j];
				col++;
			}
		if (pid)
			for (int i = 0; i < 36; i++) d.PU[i] = (i % 7 == 0) ? 1.0 : 0.0;
	}
	d.in_frame = c.parametrization_in_compliant_frame;
	for (int i = 0; i < 3; i++) {
		d.kp_pos[i] = c.kp_pos[i], d.kv_pos[i] = c.kv_pos[i], d.ki_pos[i] = c.ki_pos[i];
		d.kp_ori[i] = c.kp_ori[i], d.kv_ori[i] = c.kv_ori[i], d.ki_ori[i] = c.ki_ori[i];
		d.kp_f[i] = c.kp_force[i], d.kv_f[i] = c.kv_force[i], d.ki_f[i] = c.ki_force[i];
		d.kp_m[i] = c.kp_moment[i], d.kv_m[i] = c.kv_moment[i], d.ki_m[i] = c.ki_moment[i];
		d.faxis[i] = c.force_axis[i], d.maxis[i] = c.moment_axis[i];
		d.sensor_pos[i] = c.sensor_pos[i];
	}
	std::memcpy(d.sensor_rot, c.sensor_rot, sizeof(d.sensor_rot));
	d.kff_f = c.kff_force, d.kff_m = c.kff_moment, d.max_f = c.max_force_feedback, d.max_m = c.max_moment_feedback;
	d.cl_force = c.closed_loop_force, d.cl_moment = c.closed_loop_moment;
	d.passivity = c.passivity_enabled;
	d.fdim = c.force_space_dimension, d.mdim = c.moment_space_dimension;
	d.lin_vsat = c.linear_saturation_velocity, d.ang_vsat = c.angular_saturation_velocity;
	d.plain_motion = (d.full_projection && d.fdim == 0 && d.mdim == 0 && !d.use_vsat) ? 1 : 0;
	// MotionForceTask.cpp:892-971 with rotation = identity (world-frame parametrisation)
	for (int blk = 0; blk < 2; blk++) {
		const int dim = blk ? c.moment_space_dimension : c.force_space_dimension;
		const double* ax = blk ? c.moment_axis : c.force_axis;
		double Pb[9], A[9], T[9], sf[9], sp[9];
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) {
				Pb[3 * i + j] = c.partial_projection[(3 * blk + i) * 6 + 3 * blk + j];
				const double aa = ax[i] * ax[j], id = i == j ? 1.0 : 0.0;
				A[3 * i + j] = dim == 1 ? aa : (dim == 2 ? id - aa : (dim == 3 ? id : 0.0));
			}
		auto mul = [](const double* X, const double* Y, bool yt, double* Z) {
			for (int i = 0; i < 3; i++)
				for (int j = 0; j < 3; j++) {
					double v = 0;
					for (int k = 0; k < 3; k++) v += X[3 * i + k] * (yt ? Y[3 * j + k] : Y[3 * k + j]);
					Z[3 * i + j] = v;
				}
		};
		mul(Pb, A, false, T);
		mul(T, Pb, true, sf);
		if (dim == 3) std::memcpy(sf, Pb, sizeof(sf));
		for (int i = 0; i < 9; i++) A[i] = (i % 4 == 0 ? 1.0 : 0.0) - sf[i];
		mul(Pb, A, false, T);
		mul(T, Pb, true, sp);
		std::memcpy(d.sig[2 * blk], sf, sizeof(sf));
		std::memcpy(d.sig[2 * blk + 1], sp, sizeof(sp));
	}
	d.s_min = c.s_min, d.s_max = c.s_max, d.s_abs_tol = c.s_abs_tol, d.type_1_tol = c.type_1_tol;
	d.t2_ratio = c.type_2_torque_ratio, d.t2_angle = c.type_2_angle_threshold, d.perturb = c.perturb_step_size;
	d.sh_cap = c.sh_buffer_size;
	d.kp1 = c.kp_type_1, d.kv1 = c.kv_type_1, d.kv2 = c.kv_type_2;
	d.enforce_t1 = c.enforce_type_1_strategy, d.enforce = c.enforce_handling_strategy;
	d.sv_sign = c.singular_vector_sign;
	// internal OTG: one generator DoF per task dof (JT) or 3 linear + 3 angular (MFT)
	d.otg_on = c.use_internal_otg ? 1 : 0;
	d.otg_jerk = (c.use_internal_otg && c.internal_otg_jerk_limited) ? 1 : 0;
	d.otg_n = c.type == SAI2B_JOINT_TASK ? c.task_dof : 6;
	for (int i = 0; i < sai2b::OTG_MD; i++) {
		if (c.type == SAI2B_JOINT_TASK) {
			d.otg_vmax[i] = i < c.task_dof ? c.otg_max_velocity[i] : 0.0;
			d.otg_amax[i] = i < c.task_dof ? c.otg_max_acceleration[i] : 0.0;
			d.otg_jmax[i] = i < c.task_dof ? c.otg_max_jerk[i] : 0.0;
		} else {
			d.otg_vmax[i] = i < 3 ? c.otg_max_linear_velocity : i < 6 ? c.otg_max_angular_velocity : 0.0;
			d.otg_amax[i] = i < 3 ? c.otg_max_linear_acceleration : i < 6 ? c.otg_max_angular_acceleration : 0.0;
			d.otg_jmax[i] = i < 3 ? c.otg_max_linear_jerk : i < 6 ? c.otg_max_angular_jerk : 0.0;
		}
	}
}

template <class T>
static int dev_alloc(sai2b_ctx* ctx, T** p, size_t count) {
	void* v = nullptr;
	HIP_TRY(ctx, hipMalloc(&v, std::max<size_t>(count, 1) * sizeof(T)));
	HIP_TRY(ctx, hipMemsetAsync(v, 0, std::max<size_t>(count, 1) * sizeof(T), ctx->stream));
	ctx->allocs.push_back(v);
	*p = (T*)v;
	return SAI2B_OK;
}

// POPCExplicitForceControl::reInitialize (POPCExplicitForceControl.cpp:10-22) for every robot of a task;
// buffers are created on first use (1024-sample window ring per robot)
static int popc_reinit(sai2b_ctx* ctx, int task) {
	DevTask& d = ctx->h_params.task[task];
	const size_t B = ctx->B;
	int rc;
	if (!d.popc_f) {
		if ((rc = dev_alloc(ctx, &d.popc_f, 4 * B))) return rc;
		if ((rc = dev_alloc(ctx, &d.popc_i, 3 * B))) return rc;
		if ((rc = dev_alloc(ctx, &d.popc_q, (size_t)sai2b::POPC_RING * B))) return rc;
		ctx->params_dirty = true;
	}
	std::vector<double> f(4 * B, 0.0);
	std::fill(f.begin() + 3 * B, f.end(), 1.0);	 // Rc = 1
	std::vector<int> iv(3 * B, 0);
	std::fill(iv.begin(), iv.begin() + B, sai2b::POPC_MAX_COUNTER);
	HIP_TRY(ctx, hipMemcpyAsync(d.popc_f, f.data(), f.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(d.popc_i, iv.data(), iv.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

static int upload_params(sai2b_ctx* ctx) {
	if (!ctx->params_dirty) return SAI2B_OK;
	ctx->h_params.any_bie = 0, ctx->h_params.bie_thr = 0;
	for (int t = 0; t < ctx->h_params.n_tasks; t++)
		if (ctx->h_params.task[t].decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES) {
			ctx->h_params.any_bie = 1;
			ctx->h_params.bie_thr = ctx->h_params.task[t].bie_threshold;
		}
	// the headline body's block of copies: written here and nowhere else, from what is about to be sent
	sai2b::fast_block_fill(ctx->h_params);
	// stream-ordered so that kernels already enqueued keep the parameters they were launched with
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_params, &ctx->h_params, sizeof(DevParams), hipMemcpyHostToDevice, ctx->stream));
	DevParams meas;
	if (ctx->js_on) {  // the same parameters with the measured pair as their state
		meas = ctx->h_params;
		meas.q = ctx->js_qm, meas.dq = ctx->js_dqm;
		sai2b::fast_block_fill(meas);
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_params_meas, &meas, sizeof(DevParams), hipMemcpyHostToDevice, ctx->stream));
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // h_params may be edited again right after
	ctx->params_dirty = false;
	return SAI2B_OK;
}

static int create_impl(sai2b_ctx* ctx, const sai2b_robot_model* model, const sai2b_task_config* tasks, int n_tasks,
					   int batch, int device) {
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "sai2b_create: no HIP device available (this library has no CPU path)");
	if (device < 0 || device >= ndev) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_create: bad device index");
	HIP_TRY(ctx, hipSetDevice(device));
	HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
	HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming));
	HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_out, hipEventDisableTiming));
	ctx->B = batch, ctx->T = n_tasks, ctx->device = device;
	ctx->model = *model;
	ctx->sw = sai2b::route_switches_from_env();
	ctx->route = sai2b::TickRoute(ctx->sw);
	ctx->blocking_sync = sai2b::env_flag("SAI2B_BLOCKING_SYNC");
	ctx->no_otg_idle_skip = sai2b::env_flag("SAI2B_NO_OTG_IDLE_SKIP");
	DevParams& hp = ctx->h_params;
	std::memset(&hp, 0, sizeof(hp));
	hp.B = batch, hp.n_tasks = n_tasks;
	sai2b::host_fill_dev_model(*model, hp.model);
	if constexpr (N == 7) {
		using PB = sai2b::PandaBaked;
		const DevModel& m = hp.model;
		ctx->baked_model = std::memcmp(m.E, PB::E, sizeof(m.E)) == 0 && std::memcmp(m.xyz, PB::xyz, sizeof(m.xyz)) == 0 &&
						   std::memcmp(m.mass, PB::mass, sizeof(m.mass)) == 0 && std::memcmp(m.com, PB::com, sizeof(m.com)) == 0 &&
						   std::memcmp(m.inertia, PB::inertia, sizeof(m.inertia)) == 0 &&
						   std::memcmp(m.gravity, PB::gravity, sizeof(m.gravity)) == 0 &&
						   std::memcmp(m.jtype, PB::jtype, sizeof(m.jtype)) == 0;
		if (sai2b::env_flag("SAI2B_NO_BAKED_MODEL")) ctx->baked_model = false;
	}
	const size_t Bs = (size_t)batch;
	int rc;
	if ((rc = dev_alloc(ctx, &ctx->d_params, 1))) return rc;
	if ((rc = dev_alloc(ctx, &ctx->q, N * Bs))) return rc;
	if ((rc = dev_alloc(ctx, &ctx->dq, N * Bs))) return rc;
	if ((rc = dev_alloc(ctx, &ctx->tau, N * Bs))) return rc;
	hp.q = ctx->q, hp.dq = ctx->dq, hp.tau = ctx->tau;
	if ((rc = dev_alloc(ctx, &ctx->q_pose, (size_t)N * Bs))) return rc;
	if ((rc = dev_alloc(ctx, &ctx->fb.counts, 6))) return rc;
	HIP_TRY(ctx, hipHostMalloc((void**)&ctx->fb_report, 3 * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
	ctx->fb_report[0] = ctx->fb_report[1] = ctx->fb_report[2] = 0;
	HIP_TRY(ctx, hipHostGetDevicePointer((void**)&ctx->fb.report, ctx->fb_report, 0));
	if ((rc = dev_alloc(ctx, &ctx->fb.list, Bs))) return rc;
	if ((rc = dev_alloc(ctx, &ctx->rg.counts, 2))) return rc;
	if ((rc = dev_alloc(ctx, &ctx->rg.list, Bs))) return rc;
	HIP_TRY(ctx, hipHostMalloc((void**)&ctx->fb_seen, 2 * sizeof(int), hipHostMallocDefault));
	ctx->fb_seen[0] = ctx->fb_seen[1] = 0;
	HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->fb_seen_ev, hipEventDisableTiming));
	if ((rc = dev_alloc(ctx, &ctx->otg.counts, 2 * SAI2B_MAX_TASKS + 2))) return rc;  // (+ 2: non-idle robots of a tick, alternating)
	HIP_TRY(ctx, hipHostMalloc((void**)&ctx->otg_busy_seen, sizeof(int), hipHostMallocDefault));
	*ctx->otg_busy_seen = 1;
	HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->otg_seen_ev, hipEventDisableTiming));
	if ((rc = dev_alloc(ctx, &ctx->otg.list, SAI2B_MAX_TASKS * Bs))) return rc;
	for (int t = 0; t < n_tasks; t++) {
		ctx->cfg[t] = tasks[t];
		normalise_axes(ctx->cfg[t]);
		DevTask& d = hp.task[t];
		fill_dev_task(ctx->cfg[t], d);
		if (tasks[t].type == SAI2B_MOTION_FORCE_TASK) {
			if ((rc = dev_alloc(ctx, &d.goals, sai2b::MFT_GOAL_ROWS * Bs))) return rc;
			if ((rc = dev_alloc(ctx, &d.sensed, 6 * Bs))) return rc;
			if ((rc = dev_alloc(ctx, &d.state, sai2b::MFT_STATE_ROWS * Bs))) return rc;
			if ((rc = dev_alloc(ctx, &d.istate, sai2b::MFT_ISTATE_ROWS * Bs))) return rc;
		} else {
			if ((rc = dev_alloc(ctx, &d.goals, 3 * (size_t)d.k0 * Bs))) return rc;
			if ((rc = dev_alloc(ctx, &d.state, (size_t)d.k0 * Bs))) return rc;
		}
		// the OTG objects exist (and follow reinitialize) whether or not the OTG is enabled
		const size_t goal_rows = tasks[t].type == SAI2B_MOTION_FORCE_TASK ? (size_t)sai2b::MFT_GOAL_ROWS : 3 * (size_t)d.k0;
		if ((rc = dev_alloc(ctx, &d.otg_desired, goal_rows * Bs))) return rc;
		if ((rc = dev_alloc(ctx, &d.otg_state, (size_t)sai2b::OTG_ROWS * Bs))) return rc;
		d.otg3_traj = nullptr;
		if (d.otg_jerk && (rc = dev_alloc(ctx, &d.otg3_traj, (size_t)sai2b::OTG_MD * sai2b::OTG3_STRIDE * Bs))) return rc;
		d.otg_epoch = 0.0;
		d.otg_out_is_desired = (tasks[t].type == SAI2B_JOINT_TASK && d.k0 == N && N == sai2b::OTG_MD) ? 1 : 0;  // same row stride
		d.law_goals = d.otg_on ? (d.otg_out_is_desired ? d.otg_state + (size_t)sai2b::OTG_OUT * Bs : d.otg_desired) : d.goals;
	}
	for (int t = 0; t < n_tasks; t++)
		if (tasks[t].type == SAI2B_MOTION_FORCE_TASK && tasks[t].passivity_enabled && (rc = popc_reinit(ctx, t))) return rc;
	ctx->params_dirty = true;
	if ((rc = upload_params(ctx))) return rc;
	// the reference constructs tasks from the model's current state (q = 0 until set_state)
	if (sai2b::launch_reinit(ctrl_params(ctx), ctx->B, -1, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "reinit launch failed");
	if (sai2b::launch_otg_reinit(ctrl_params(ctx), ctx->B, -1, 0, ctx->q, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "OTG reinit launch failed");
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

extern "C" sai2b_ctx* sai2b_create(const sai2b_robot_model* model, const sai2b_task_config* tasks, int n_tasks, int batch,
								   int device) {
	if (!model || model->dof != N) {
		set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_create: robot model has a number of joints this library was not built for");
		return nullptr;
	}
	for (int i = 0; i < N; i++)
		if (model->joint_type[i] != SAI2B_REVOLUTE && model->joint_type[i] != SAI2B_PRISMATIC) {
			set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_create: joint_type must be SAI2B_REVOLUTE or SAI2B_PRISMATIC");
			return nullptr;
		}
	if (batch < 1) {
		set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_create: batch must be >= 1");
		return nullptr;
	}
	char msg[256];
	if (sai2b_validate_tasks(tasks, n_tasks, msg, sizeof(msg))) return nullptr;
	sai2b_ctx* ctx = new sai2b_ctx();
	if (create_impl(ctx, model, tasks, n_tasks, batch, device) != SAI2B_OK) {
		std::string keep = ctx->error;
		sai2b_destroy(ctx);
		g_error = keep;
		return nullptr;
	}
	return ctx;
}

extern "C" void sai2b_destroy(sai2b_ctx* ctx) {
	if (!ctx) return;
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	for (void* p : ctx->allocs) (void)hipFree(p);
	if (ctx->ev_in) (void)hipEventDestroy(ctx->ev_in);
	if (ctx->ev_out) (void)hipEventDestroy(ctx->ev_out);
	if (ctx->fb_seen_ev) (void)hipEventDestroy(ctx->fb_seen_ev);
	if (ctx->otg_seen_ev) (void)hipEventDestroy(ctx->otg_seen_ev);
	if (ctx->otg_busy_seen) (void)hipHostFree(ctx->otg_busy_seen);
	if (ctx->fb_seen) (void)hipHostFree(ctx->fb_seen);
	if (ctx->fb_report) (void)hipHostFree(ctx->fb_report);
	if (ctx->snap_report) (void)hipHostFree(ctx->snap_report);
	if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
	delete ctx;
}

extern "C" const char* sai2b_last_error(const sai2b_ctx* ctx) { return ctx ? ctx->error.c_str() : g_error.c_str(); }
extern "C" int sai2b_batch(const sai2b_ctx* ctx) { return ctx ? ctx->B : 0; }
extern "C" int sai2b_num_tasks(const sai2b_ctx* ctx) { return ctx ? ctx->T : 0; }
extern "C" int sai2b_num_joints(const sai2b_ctx* ctx) { return ctx ? N : 0; }

// `reset` of MotionForceTask::parametrizeForceMotionSpaces / parametrizeMomentRotMotionSpaces
// (MotionForceTask.cpp:838-848,866-878): the dimension changed, or, for dimension 1 or 2, the normalised
// axis is not isApprox (Eigen default 1e-12) the one in use
static bool space_changed(int dim, const double* axis, int old_dim, const double* old_axis) {
	if (dim != old_dim) return true;
	if (dim != 1 && dim != 2) return false;
	double na = 0, nb = 0, d2 = 0, a2 = 0, b2 = 0;
	for (int i = 0; i < 3; i++) na += axis[i] * axis[i], nb += old_axis[i] * old_axis[i];
	na = std::sqrt(na), nb = std::sqrt(nb);
	for (int i = 0; i < 3; i++) {
		const double a = axis[i] / na, b = old_axis[i] / nb;
		d2 += (a - b) * (a - b), a2 += a * a, b2 += b * b;
	}
	return !(d2 <= 1e-24 * std::min(a2, b2));
}

extern "C" int sai2b_update_task_config(sai2b_ctx* ctx, int task, const sai2b_task_config* cfg) {
	if (!ctx || !cfg || task < 0 || task >= ctx->T) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_update_task_config: bad arguments");
	if (int rc_ = flush_update(ctx)) return rc_;
	const sai2b_task_config& old = ctx->cfg[task];
	if (cfg->type != old.type || cfg->task_dof != old.task_dof || cfg->link != old.link ||
		std::memcmp(cfg->joint_selection, old.joint_selection, sizeof(old.joint_selection)) != 0 ||
		std::memcmp(cfg->partial_projection, old.partial_projection, sizeof(old.partial_projection)) != 0)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_update_task_config: structural fields must not change");
	sai2b_task_config all[SAI2B_MAX_TASKS];
	for (int t = 0; t < ctx->T; t++) all[t] = ctx->cfg[t];
	all[task] = *cfg;
	char msg[256];
	if (sai2b_validate_tasks(all, ctx->T, msg, sizeof(msg))) return set_error(ctx, SAI2B_INVALID_ARGUMENT, msg);
	const bool popc_toggle = old.type == SAI2B_MOTION_FORCE_TASK && (cfg->passivity_enabled != 0) != (old.passivity_enabled != 0);
	int reparam = 0;  // flags of mft_reparam_kernel
	if (old.type == SAI2B_MOTION_FORCE_TASK) {
		const bool lin = space_changed(cfg->force_space_dimension, cfg->force_axis, old.force_space_dimension, old.force_axis);
		const bool ang = space_changed(cfg->moment_space_dimension, cfg->moment_axis, old.moment_space_dimension, old.moment_axis);
		const bool cl_f = (cfg->closed_loop_force != 0) != (old.closed_loop_force != 0);
		const bool cl_m = (cfg->closed_loop_moment != 0) != (old.closed_loop_moment != 0);
		reparam = (lin ? 1 | 4 : 0) | (ang ? 2 | 8 : 0) | (cl_f ? 4 : 0) | (cl_m ? 8 : 0);
	}
	ctx->cfg[task] = *cfg;
	normalise_axes(ctx->cfg[task]);
	DevTask& d = ctx->h_params.task[task];
	DevTask keep = d;
	fill_dev_task(ctx->cfg[task], d);
	d.popc_f = keep.popc_f, d.popc_i = keep.popc_i, d.popc_q = keep.popc_q;
	// enable(): just switches on; disable(): also reinitialises (POPCExplicitForceControl.cpp:24-28).
	// Buffers must exist before the first enabled tick.
	if (popc_toggle || (cfg->passivity_enabled && !d.popc_f)) {
		int rc2 = popc_reinit(ctx, task);
		if (rc2) return rc2;
	}
	d.goals = keep.goals, d.sensed = keep.sensed, d.state = keep.state, d.istate = keep.istate;
	d.dbg_tau = keep.dbg_tau, d.dbg_N = keep.dbg_N, d.dbg_sigma = keep.dbg_sigma, d.dbg_J = keep.dbg_J, d.dbg_pose = keep.dbg_pose;
	d.dbg_F = keep.dbg_F;
	d.otg_desired = keep.otg_desired, d.otg_state = keep.otg_state, d.otg_epoch = keep.otg_epoch;
	d.otg3_traj = keep.otg3_traj;
	if (d.otg_jerk && !d.otg3_traj) {
		int rc5 = dev_alloc(ctx, &d.otg3_traj, (size_t)sai2b::OTG_MD * sai2b::OTG3_STRIDE * (size_t)ctx->B);
		if (rc5) return rc5;
	}
	d.otg_out_is_desired = keep.otg_out_is_desired, d.otg_gated = keep.otg_gated;
	d.law_goals = d.otg_on ? (d.otg_out_is_desired ? d.otg_state + (size_t)sai2b::OTG_OUT * ctx->B : d.otg_desired) : d.goals;
	ctx->params_dirty = true;
	ctx->goals_dirty |= 1u << task;
	ctx->goals_epoch++, ctx->otg_all_idle = false;
	// enableInternalOtgAccelerationLimited (JointTask.cpp:360-381, MotionForceTask.cpp:511-523) is
	// applied when the OTG fields change: new limits make every moving robot re-plan
	// (InputParameter::operator!=, input_parameter.hpp:362-394); a generator that was off is
	// re-initialised at the current state first
	// enableInternalOtgJerkLimited (JointTask.cpp:383-406, MotionForceTask.cpp:525-538) likewise; a generator that is on and
	// changes its kind of limitation (getJerkLimitEnabled() differs) restarts at the task's current pose too, and
	// setMaxJerk, unlike disableJerkLimits, does not touch the input acceleration
	const bool mode_changed = keep.otg_on && d.otg_jerk != keep.otg_jerk;
	const bool limits_changed = std::memcmp(d.otg_vmax, keep.otg_vmax, sizeof(d.otg_vmax)) != 0 ||
								std::memcmp(d.otg_amax, keep.otg_amax, sizeof(d.otg_amax)) != 0 ||
								(d.otg_jerk && std::memcmp(d.otg_jmax, keep.otg_jmax, sizeof(d.otg_jmax)) != 0);
	if (d.otg_on && (limits_changed || mode_changed || !keep.otg_on)) {
		if (limits_changed || mode_changed) d.otg_epoch += 1.0;
		const int reinit_mode = (!keep.otg_on || mode_changed) ? 1 : (d.otg_jerk ? -1 : 2);
		int rc3 = upload_params(ctx);
		if (rc3) return rc3;
		if (reinit_mode >= 0) {
			if (sai2b::launch_otg_reinit(ctrl_params(ctx), ctx->B, task, reinit_mode, ctx->q_is_pose ? ctrl_q(ctx) : ctx->q_pose, ctx->stream))
				return set_error(ctx, SAI2B_RUNTIME_ERROR, "OTG enable launch failed");
			ctx->launches++;
		}
	}
	if (reparam) {
		int rc4 = upload_params(ctx);
		if (rc4) return rc4;
		if (sai2b::launch_mft_reparam(ctrl_params(ctx), ctx->B, task, reparam, ctx->q_is_pose ? ctrl_q(ctx) : ctx->q_pose, ctx->stream))
			return set_error(ctx, SAI2B_RUNTIME_ERROR, "re-parametrisation launch failed");
		ctx->launches++;
	}
	return SAI2B_OK;
}

extern "C" int sai2b_enable_gravity_compensation(sai2b_ctx* ctx, int enable) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;
	ctx->h_params.gravity_comp = enable ? 1 : 0;
	ctx->params_dirty = true;
	return SAI2B_OK;
}

// Ordering of device-pointer arguments against the caller's stream. before_read: work the caller enqueued on its
// stream so far (the producer of the argument) completes before what the ctx stream does next; after_read: what
// the ctx stream has been given so far (the read of the argument, or the write of a device result) completes
// before anything the caller enqueues on its stream afterwards — so the caller may overwrite an input, or
// consume a result, right after the call returns without synchronising.
static int caller_before_read(sai2b_ctx* ctx) {
	HIP_TRY(ctx, hipEventRecord(ctx->ev_in, ctx->caller_stream));
	HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
	return SAI2B_OK;
}
static int caller_after_read(sai2b_ctx* ctx) {
	HIP_TRY(ctx, hipEventRecord(ctx->ev_out, ctx->stream));
	HIP_TRY(ctx, hipStreamWaitEvent(ctx->caller_stream, ctx->ev_out, 0));
	return SAI2B_OK;
}

static int copy_rows(sai2b_ctx* ctx, double* dst, const double* src, size_t rows, int on_device) {
	if (!src) return SAI2B_OK;
	int rc;
	if (on_device && (rc = caller_before_read(ctx))) return rc;
	HIP_TRY(ctx, hipMemcpyAsync(dst, src, rows * (size_t)ctx->B * sizeof(double),
								on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
	if (on_device) return caller_after_read(ctx);
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // pageable host memory may be reused by the caller
	return SAI2B_OK;
}

// called before the state buffers are overwritten
static int keep_pose(sai2b_ctx* ctx) {
	if (!ctx->q_is_pose) return SAI2B_OK;
	HIP_TRY(ctx, hipMemcpyAsync(ctx->q_pose, ctrl_q(ctx), sizeof(double) * N * (size_t)ctx->B, hipMemcpyDeviceToDevice, ctx->stream));
	ctx->q_is_pose = false;
	return SAI2B_OK;
}

// joint sensors: what joint_sense_kernel takes from the context
static sai2b::JointSenseParams joint_sense_params(const sai2b_ctx* ctx) {
	sai2b::JointSenseParams p;
	p.rows = ctx->js_rows, p.q = ctx->q, p.dq = ctx->dq, p.q_meas = ctx->js_qm, p.dq_meas = ctx->js_dqm;
	p.prev = ctx->js_prev, p.filter = ctx->js_filter, p.history = ctx->js_history, p.clock = ctx->js_clock;
	p.depth = ctx->js_cfg.max_delay, p.velocity_mode = ctx->js_cfg.velocity_mode;
	p.rng.key0 = (unsigned)(ctx->js_cfg.seed & 0xffffffffull), p.rng.key1 = (unsigned)(ctx->js_cfg.seed >> 32);
	p.rng.first_robot = ctx->js_cfg.first_robot;
	return p;
}
// reading 0 of the truth as it is on the stream, for the robots of `mask` (device bytes; NULL: all). The measured q is about to be
// overwritten: while it is the tasks' cached pose it is saved first.
static int joint_sensor_seed(sai2b_ctx* ctx, const unsigned char* mask, bool next_episode) {
	if (int rc = keep_pose(ctx)) return rc;
	sai2b::JointSenseParams p = joint_sense_params(ctx);
	p.mask = mask, p.next_episode = next_episode ? 1 : 0;
	if (sai2b::launch_joint_sense(ctx->B, p, true, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "joint sensor seed launch failed");
	ctx->launches++;
	return SAI2B_OK;
}

extern "C" int sai2b_set_state(sai2b_ctx* ctx, const double* q, const double* dq, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc;
	if (q && (rc = keep_pose(ctx))) return rc;
	if ((rc = copy_rows(ctx, ctx->q, q, N, on_device))) return rc;
	if ((rc = copy_rows(ctx, ctx->dq, dq, N, on_device))) return rc;
	// joint sensors: the state was set, not measured: every robot's measurement starts again at reading 0 of its episode
	if (ctx->js_on && (q || dq) && (rc = joint_sensor_seed(ctx, nullptr, false))) return rc;
	ctx->models_fresh = false;
	for (int t = 0; t < ctx->T; t++) ctx->tio[t].model_fresh = false;
	return SAI2B_OK;
}

static int mft_task_check(sai2b_ctx* ctx, int task, const char* fn) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (task < 0 || task >= ctx->T || ctx->cfg[task].type != SAI2B_MOTION_FORCE_TASK)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string(fn) + ": task is not a MotionForceTask");
	return hipSetDevice(ctx->device) == hipSuccess ? SAI2B_OK : set_error(ctx, SAI2B_RUNTIME_ERROR, "hipSetDevice failed");
}

extern "C" int sai2b_set_mft_goals(sai2b_ctx* ctx, int task, const double* pos, const double* rot, const double* lin_vel,
								   const double* ang_vel, const double* lin_acc, const double* ang_acc, int on_device) {
	int rc = mft_task_check(ctx, task, "sai2b_set_mft_goals");
	if (rc) return rc;
	double* G = ctx->h_params.task[task].goals;
	const size_t B = ctx->B;
	ctx->goals_dirty |= 1u << task;
	ctx->goals_epoch++, ctx->otg_all_idle = false;
	if ((rc = copy_rows(ctx, G + sai2b::MFT_GOAL_POS * B, pos, 3, on_device))) return rc;
	if ((rc = copy_rows(ctx, G + sai2b::MFT_GOAL_ROT * B, rot, 9, on_device))) return rc;
	if ((rc = copy_rows(ctx, G + sai2b::MFT_GOAL_LIN_VEL * B, lin_vel, 3, on_device))) return rc;
	if ((rc = copy_rows(ctx, G + sai2b::MFT_GOAL_ANG_VEL * B, ang_vel, 3, on_device))) return rc;
	if ((rc = copy_rows(ctx, G + sai2b::MFT_GOAL_LIN_ACC * B, lin_acc, 3, on_device))) return rc;
	return copy_rows(ctx, G + sai2b::MFT_GOAL_ANG_ACC * B, ang_acc, 3, on_device);
}

extern "C" int sai2b_set_mft_goal_wrench(sai2b_ctx* ctx, int task, const double* force, const double* moment, int on_device) {
	int rc = mft_task_check(ctx, task, "sai2b_set_mft_goal_wrench");
	if (rc) return rc;
	double* G = ctx->h_params.task[task].goals;
	const size_t B = ctx->B;
	if ((rc = copy_rows(ctx, G + sai2b::MFT_GOAL_FORCE * B, force, 3, on_device))) return rc;
	return copy_rows(ctx, G + sai2b::MFT_GOAL_MOMENT * B, moment, 3, on_device);
}

extern "C" int sai2b_set_mft_sensed_wrench(sai2b_ctx* ctx, int task, const double* force, const double* moment, int on_device) {
	int rc = mft_task_check(ctx, task, "sai2b_set_mft_sensed_wrench");
	if (rc) return rc;
	double* S = ctx->h_params.task[task].sensed;
	if ((rc = copy_rows(ctx, S, force, 3, on_device))) return rc;
	return copy_rows(ctx, S + 3 * (size_t)ctx->B, moment, 3, on_device);
}

extern "C" int sai2b_set_jt_goals(sai2b_ctx* ctx, int task, const double* q_goal, const double* dq_goal, const double* ddq_goal,
								  int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (task < 0 || task >= ctx->T || ctx->cfg[task].type != SAI2B_JOINT_TASK)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_jt_goals: task is not a JointTask");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	double* G = ctx->h_params.task[task].goals;
	const size_t B = ctx->B, k0 = ctx->cfg[task].task_dof;
	ctx->goals_dirty |= 1u << task;
	ctx->goals_epoch++, ctx->otg_all_idle = false;
	int rc;
	if ((rc = copy_rows(ctx, G, q_goal, k0, on_device))) return rc;
	if ((rc = copy_rows(ctx, G + k0 * B, dq_goal, k0, on_device))) return rc;
	return copy_rows(ctx, G + 2 * k0 * B, ddq_goal, k0, on_device);
}

extern "C" int sai2b_reinitialize(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = upload_params(ctx);
	if (rc) return rc;
	if (sai2b::launch_reinit(ctrl_params(ctx), ctx->B, -1, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "reinit launch failed");
	if (sai2b::launch_otg_reinit(ctrl_params(ctx), ctx->B, -1, 0, ctx->q, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "OTG reinit launch failed");
	ctx->goals_dirty = ~0u;
	ctx->goals_epoch++, ctx->otg_all_idle = false;
	ctx->launches += 2;
	ctx->models_fresh = false;
	ctx->q_is_pose = true;	// reInitializeTask reads the pose of the current state
	return SAI2B_OK;
}

// sai2b_reinitialize_robots (episode = false) and sai2b_reset_robots (episode = true): one launch of reset_subset_kernel
// and sai2b_reset_robots_sampled (episode and sampled = true, q and dq NULL): one launch of reset_sampled_kernel in its place
static sai2b::RsParams reset_sampler_params(const sai2b_ctx* ctx);
static int reset_subset(sai2b_ctx* ctx, const char* fn, int task, const unsigned char* mask, const double* q, const double* dq, int on_device,
						bool episode, bool sampled = false) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, std::string(fn) + ": null ctx");
	if (sampled && !ctx->rs_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string(fn) + ": no reset sampler is configured (sai2b_set_reset_sampler)");
	if (!mask) return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string(fn) + ": mask is NULL");
	if (sampled && ctx->rs_cfg.use_clearance && !ctx->h_params.contact)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string(fn) + ": reset sampler: use_clearance needs a contact (sai2b_set_contact)");
	if (task < -1 || task >= ctx->T) return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string(fn) + ": task must be -1 (every task) or a task index");
	if (int rc_ = flush_update(ctx)) return rc_;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = upload_params(ctx);
	if (rc) return rc;
	const size_t B = ctx->B;
	const unsigned char* d_mask = mask;
	const double *d_q = q, *d_dq = dq;
	if (on_device) {
		if ((rc = caller_before_read(ctx))) return rc;
	} else {
		if (!ctx->reset_mask && (rc = dev_alloc(ctx, &ctx->reset_mask, B))) return rc;
		if ((q || dq) && !ctx->reset_rows && (rc = dev_alloc(ctx, &ctx->reset_rows, 2 * (size_t)N * B))) return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->reset_mask, mask, B, hipMemcpyHostToDevice, ctx->stream));
		d_mask = ctx->reset_mask;
		if (q) {
			HIP_TRY(ctx, hipMemcpyAsync(ctx->reset_rows, q, (size_t)N * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
			d_q = ctx->reset_rows;
		}
		if (dq) {
			HIP_TRY(ctx, hipMemcpyAsync(ctx->reset_rows + (size_t)N * B, dq, (size_t)N * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
			d_dq = ctx->reset_rows + (size_t)N * B;
		}
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // pageable host memory may be reused by the caller
	}
	// q_is_pose is one flag for the batch. While it holds, the state buffer is every robot's cached pose and stays so: a
	// selected robot's new state is the pose it is re-initialised at. Otherwise the unselected robots' poses live in q_pose
	// and the kernel moves the selected columns there (one task of several: the other tasks keep theirs, as
	// sai2b_task_reinitialize has it).
	// Joint sensors: a reset (episode) runs on the true view, so a selected robot's tasks are re-initialised at its true start
	// state, and the seeding launch behind it takes its first measurement; a re-initialisation alone reads the measured view.
	// While q_is_pose holds the cached pose of the robots left alone is the measured q, which is no state a reset robot could be
	// re-initialised at: the pose moves to q_pose first, and the kernel puts the selected robots' true start there.
	const bool true_view = ctx->js_on && episode;
	if (true_view && (rc = keep_pose(ctx))) return rc;
	const DevParams* view = true_view ? ctx->d_params : ctrl_params(ctx);
	double *q_state = true_view ? ctx->q : ctrl_q(ctx), *dq_state = true_view ? ctx->dq : ctrl_dq(ctx);
	int flags = episode ? sai2b::RESET_EPISODE : 0;
	if (!ctx->q_is_pose && (task < 0 || ctx->T == 1)) flags |= sai2b::RESET_KEEP_POSE;
	if (sampled) {
		HIP_TRY(ctx, hipMemsetAsync(ctx->rs_counts, 0, sai2b::RS_COUNTS * sizeof(int), ctx->stream));
		if (sai2b::launch_reset_sampled(view, ctx->B, reset_sampler_params(ctx), d_mask, q_state, dq_state, ctx->q_pose,
										flags & sai2b::RESET_KEEP_POSE, ctx->stream))
			return set_error(ctx, SAI2B_RUNTIME_ERROR, std::string(fn) + ": launch failed");
	} else if (sai2b::launch_reset_subset(view, ctx->B, d_mask, d_q, d_dq, q_state, dq_state, ctx->q_pose, task, flags, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, std::string(fn) + ": launch failed");
	// joint sensors: reading 0 of the selected robots' next episode, from the truth the reset has just written
	if (true_view && (rc = joint_sensor_seed(ctx, d_mask, true))) return rc;
	// hardware: a reset robot starts a new episode at period 0 (a re-initialisation alone leaves its clocks as they are)
	if (episode && ctx->hw_on) {
		if (sai2b::launch_hardware_reset(ctx->B, d_mask, ctx->hw_clock, ctx->stream))
			return set_error(ctx, SAI2B_RUNTIME_ERROR, std::string(fn) + ": hardware reset launch failed");
		ctx->launches++;
	}
	// reward: a reset robot starts a new return (a re-initialisation alone leaves its accumulators as they are)
	if (episode && ctx->rew_on) {
		if (sai2b::launch_reward_reset(ctx->B, d_mask, ctx->rew_state, ctx->rew_episode, ctx->stream))
			return set_error(ctx, SAI2B_RUNTIME_ERROR, std::string(fn) + ": reward reset launch failed");
		ctx->launches++;
	}
	// batch-wide and conservative: a dirty flag makes the generator kernel compare goals, and an untouched robot's compare equal
	ctx->goals_dirty = task < 0 ? ~0u : (ctx->goals_dirty | 1u << task);
	ctx->goals_epoch++, ctx->otg_all_idle = false;
	ctx->launches++;
	ctx->models_fresh = false;
	for (int t = 0; t < ctx->T; t++)
		if (task < 0 || t == task || d_q || d_dq) ctx->tio[t].model_fresh = false;
	return on_device ? caller_after_read(ctx) : SAI2B_OK;
}

extern "C" int sai2b_reset_robots_sampled(sai2b_ctx* ctx, const unsigned char* mask, int on_device) {
	return reset_subset(ctx, "sai2b_reset_robots_sampled", -1, mask, nullptr, nullptr, on_device, true, true);
}

extern "C" int sai2b_reinitialize_robots(sai2b_ctx* ctx, int task, const unsigned char* mask, int on_device) {
	return reset_subset(ctx, "sai2b_reinitialize_robots", task, mask, nullptr, nullptr, on_device, false);
}

extern "C" int sai2b_reset_robots(sai2b_ctx* ctx, const unsigned char* mask, const double* q, const double* dq, int on_device) {
	return reset_subset(ctx, "sai2b_reset_robots", -1, mask, q, dq, on_device, true);
}

// the hierarchy, the kinds of kernel it is eligible for and what a call asks for, as sai2b_tick_policy.h takes them
static sai2b::Hierarchy hierarchy(const sai2b_ctx* ctx) { return sai2b::Hierarchy{&ctx->h_params, ctx->cfg, ctx->T, ctx->model.joint_type}; }
static sai2b::RouteKinds route_kinds(const sai2b_ctx* ctx) { return sai2b::route_kinds(ctx->sw, hierarchy(ctx)); }
static sai2b::TickAsk tick_ask(const sai2b_ctx* ctx, int commit_sh, int with_comp, int do_torque, unsigned gated) {
	sai2b::TickAsk a;
	a.introspection = ctx->introspection, a.commit_sh = commit_sh, a.with_comp = with_comp, a.do_torque = do_torque;
	a.payload = ctx->h_params.payload != nullptr, a.baked = ctx->baked_model, a.gated = gated;
	return a;
}

// The counts of the pending request (launch_tick), waiting for them if they have not arrived: 0 and d / took / wmax filled, or an error
static int fb_counts_arrived(sai2b_ctx* ctx, long long* d, long long* took, long long* wmax) {
	if (ctx->route.by_copy) {
		if (hipEventQuery(ctx->fb_seen_ev) != hipSuccess) HIP_TRY(ctx, hipEventSynchronize(ctx->fb_seen_ev));
		*d = ctx->fb_seen[0], *took = ctx->fb_seen[1], *wmax = -1;
		return SAI2B_OK;
	}
	const unsigned long long want = ctx->route.stamp;
	unsigned long long w0 = 0, w1 = 0, w2 = 0;
	auto arrived = [&] {
		w0 = __atomic_load_n(&ctx->fb_report[0], __ATOMIC_ACQUIRE), w1 = __atomic_load_n(&ctx->fb_report[1], __ATOMIC_ACQUIRE);
		w2 = __atomic_load_n(&ctx->fb_report[2], __ATOMIC_ACQUIRE);
		return (w0 >> 32) == want && (w1 >> 32) == want && (w2 >> 32) == want;
	};
	if (!arrived()) {
		// (at a distance of 8 ticks they have, unless the caller never fetches a result)
		const auto t0 = std::chrono::steady_clock::now();
		for (unsigned spin = 0; !arrived(); spin++)
			if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
		if (!arrived()) {
			HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			if (!arrived()) return set_error(ctx, SAI2B_RUNTIME_ERROR, "the work list's counts did not reach the host");
		}
	}
	*d = (long long)(unsigned)w0, *took = (long long)(unsigned)w1, *wmax = (long long)(unsigned)w2;
	return SAI2B_OK;
}

// tasks whose generator is jerk-limited: their planner work lists take a launch of their own (sai2b_otg.hip)
static int jerk_mask(const sai2b_ctx* ctx) {
	int m = 0;
	for (int t = 0; t < ctx->T; t++)
		if (ctx->h_params.task[t].otg_on && ctx->h_params.task[t].otg_jerk) m |= 1 << t;
	return m;
}
static bool any_otg(const sai2b_ctx* ctx) {
	for (int t = 0; t < ctx->T; t++)
		if (ctx->h_params.task[t].otg_on) return true;
	return false;
}

// Which JointTasks need their generator gated per robot and tick: one whose range can come out empty
// (JointTask.cpp:233-239,302-306: the task then returns before setGoal / update of its OTG). Never the
// case for the first task (range of S) nor for an invertible selection behind fewer than 7 task DoF
// (S N_prec has the rank of N_prec >= 1, and a non-zero projector has a singular value >= 1).
static unsigned refresh_otg_gating(sai2b_ctx* ctx) {
	unsigned mask = 0;
	int dof_above = 0;
	for (int t = 0; t < ctx->h_params.n_tasks; t++) {
		DevTask& d = ctx->h_params.task[t];
		int gated = 0;
		if (d.type == SAI2B_JOINT_TASK) {
			gated = (d.otg_on && t > 0 && !(d.k0 == N && dof_above < N)) ? 1 : 0;
			// driven on its own behind a caller-supplied N_prec: nothing is known about its range
			if (ctx->tio[t].standalone) gated = (d.otg_on && ctx->tio[t].nprec_given) ? 1 : 0;
			dof_above += d.k0;
		} else {
			dof_above += d.rank;
		}
		if (d.otg_gated != gated) {
			d.otg_gated = gated;
			ctx->params_dirty = true;
		}
		if (gated) mask |= 1u << t;
	}
	return mask;
}

static int fetch_rows(sai2b_ctx* ctx, const double* src, size_t row0, size_t rows, double* dst);

static int launch_tick(sai2b_ctx* ctx, int commit_sh, int with_comp, int do_torque) {
	ctx->last_call_task = 0;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	for (int t = 0; t < ctx->T; t++) ctx->tio[t].standalone = ctx->tio[t].model_fresh = false;
	const unsigned gated = refresh_otg_gating(ctx);
	int rc = upload_params(ctx);
	if (rc) return rc;
	const sai2b::RouteKinds kinds = route_kinds(ctx);
	const sai2b::TickAsk ask = tick_ask(ctx, commit_sh, with_comp, do_torque, gated);
	// which robots' gated tasks are active this tick
	const sai2b::RangePlan range = sai2b::plan_range(ctx->route, ctx->sw, kinds, ctx->B, ask);
	if (range.run && range.cert) {
		if (sai2b::launch_range_cert(ctrl_params(ctx), ctx->B, range.max_rows, range.payload, range.inlane_singular, ctx->rg, ctx->stream) ||
			sai2b::launch_tick_group(ctrl_params(ctx), ctx->B, 16, true, false, with_comp, false, ctx->rg.count(), ctx->rg.list, ctx->stream))
			return set_error(ctx, SAI2B_RUNTIME_ERROR, "task-range pass launch failed");
		ctx->rg.parity ^= 1;
		ctx->launches += 2;
	} else if (range.run) {
		if (sai2b::launch_range_pass(ctrl_params(ctx), ctx->B, ctx->introspection, with_comp, range.lanes, ctx->stream))
			return set_error(ctx, SAI2B_RUNTIME_ERROR, "task-range pass launch failed");
		ctx->launches++;
	}
	if (do_torque && any_otg(ctx)) {  // the generators advance once per torque computation, before the law
		if (ctx->otg_look.advance()) {
			if (hipEventQuery(ctx->otg_seen_ev) != hipSuccess) HIP_TRY(ctx, hipEventSynchronize(ctx->otg_seen_ev));
			if (*ctx->otg_busy_seen == 0 && ctx->otg_obs_epoch == ctx->goals_epoch) ctx->otg_all_idle = true;
		}
		// (see otg_all_idle: exact, not a heuristic — an idle generator's update neither reads nor writes anything)
		const bool idle_skip = ctx->otg_all_idle && !gated && !ctx->goals_exposed && ctx->goals_dirty == 0 && !ctx->no_otg_idle_skip;
		if (!idle_skip) {
			// (a gated task keeps reading its goals: a robot skipped while they changed must see them later)
			const int clean_mask = ctx->goals_exposed ? 0 : (int)(~ctx->goals_dirty & ~gated & ((1u << SAI2B_MAX_TASKS) - 1u));
			ctx->goals_dirty = 0;
			if (sai2b::launch_otg(ctrl_params(ctx), ctx->B, ctx->otg, clean_mask, ~0, jerk_mask(ctx), ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "OTG launch failed");
			if (!gated && !ctx->goals_exposed && !ctx->otg_look.pending) {
				HIP_TRY(ctx, hipMemcpyAsync(ctx->otg_busy_seen, ctx->otg.counts + 2 * SAI2B_MAX_TASKS + ctx->otg.parity, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
				HIP_TRY(ctx, hipEventRecord(ctx->otg_seen_ev, ctx->stream));
				ctx->otg_look.ask();
				ctx->otg_obs_epoch = ctx->goals_epoch;
			}
			ctx->otg.parity ^= 1;
			ctx->launches += 2;
		}
	}
	// the work list's counts of 8 ticks ago, when this tick is the one to look at them
	if (sai2b::look_due(ctx->route, kinds, ask)) {
		long long d = 0, took = 0, wmax = -1;
		if (int rc_ = fb_counts_arrived(ctx, &d, &took, &wmax)) return rc_;
		sai2b::observe(ctx->route, ctx->sw, kinds, ctx->B, d, took, wmax);
	}
	const sai2b::TickPlan plan = sai2b::plan(ctx->route, ctx->sw, kinds, ctx->B, ask);
	if (plan.fast_launch) ctx->fb.parity ^= 1;
	if (sai2b::launch_tick(ctrl_params(ctx), ctx->B, plan.form, plan.call, ctx->fb, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "tick launch failed");
	ctx->launches++;
	if (plan.by_copy) {
		HIP_TRY(ctx, hipMemcpyAsync(ctx->fb_seen, ctx->fb.count(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->fb_seen + 1, ctx->fb.took(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipEventRecord(ctx->fb_seen_ev, ctx->stream));
	}
	if (do_torque) ctx->q_is_pose = true;  // computeTorques caches the tasks' current pose
	return SAI2B_OK;
}

static int fetch_tau(sai2b_ctx* ctx, double* tau, int on_device) {
	if (!tau) return SAI2B_OK;
	// a device result is written on the ctx stream: what the caller's stream still does with that buffer comes first
	if (on_device)
		if (int rc = caller_before_read(ctx)) return rc;
	HIP_TRY(ctx, hipMemcpyAsync(tau, ctx->tau, (size_t)N * ctx->B * sizeof(double),
								on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a returned tau is complete, host or device
	return SAI2B_OK;
}

// The split API recomputes the (deterministic) task models inside compute_control_torques; what
// update_task_models() adds is the once-per-tick singularity bookkeeping, which is why it is
// committed there and not again by the torque pass that follows it (DESIGN.md "split API").
static int flush_update(sai2b_ctx* ctx) {
	if (!ctx || !ctx->update_pending) return SAI2B_OK;
	ctx->update_pending = false;
	int rc = launch_tick(ctx, /*commit_sh=*/1, /*with_comp=*/1, /*do_torque=*/0);
	if (rc) return rc;
	ctx->models_fresh = true;
	return SAI2B_OK;
}
extern "C" int sai2b_update_task_models(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;  // an update still pending: it happens now, this one is the new pending one
	if (ctx->introspection) {  // the introspection outputs of the model pass are read between the two calls
		int rc = launch_tick(ctx, /*commit_sh=*/1, /*with_comp=*/1, /*do_torque=*/0);
		if (rc) return rc;
		ctx->models_fresh = true;
		return SAI2B_OK;
	}
	ctx->update_pending = true;
	return SAI2B_OK;
}

extern "C" int sai2b_compute_control_torques_ex(sai2b_ctx* ctx, double* tau, int on_device, int with_compensation) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	// a pending update is consumed here: update + torques as ONE fused tick (once-per-update singularity bookkeeping
	// committed by it, exactly as by the model pass it replaces)
	const bool fused = ctx->update_pending;
	ctx->update_pending = false;
	int rc = launch_tick(ctx, (fused || !ctx->models_fresh) ? 1 : 0, with_compensation, 1);
	if (rc) return rc;
	ctx->models_fresh = false;
	ctx->ticks += ctx->B;
	return fetch_tau(ctx, tau, on_device);
}
extern "C" int sai2b_compute_control_torques(sai2b_ctx* ctx, double* tau, int on_device) {
	return sai2b_compute_control_torques_ex(ctx, tau, on_device, 1);
}

extern "C" int sai2b_tick(sai2b_ctx* ctx, double* tau, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;
	int rc = launch_tick(ctx, 1, 1, 1);
	if (rc) return rc;
	ctx->models_fresh = false;
	ctx->ticks += ctx->B;
	return fetch_tau(ctx, tau, on_device);
}

// ------------------------------------------------------------------------------------------------
// task-level plugin interface (TemplateTask.h:42-88): one task driven on its own
// ------------------------------------------------------------------------------------------------
static int task_io(sai2b_ctx* ctx, int task, const char* fn) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (task < 0 || task >= ctx->T) return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string(fn) + ": bad task index");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (int rc_ = flush_update(ctx)) return rc_;
	sai2b_ctx::TaskIO& io = ctx->tio[task];
	if (!io.N) {
		const size_t B = ctx->B;
		int rc;
		if ((rc = dev_alloc(ctx, &io.Nprec, N * N * B))) return rc;
		if ((rc = dev_alloc(ctx, &io.N, N * N * B))) return rc;
		if ((rc = dev_alloc(ctx, &io.Ntot, N * N * B))) return rc;
		if ((rc = dev_alloc(ctx, &io.tau, N * B))) return rc;
		if ((rc = dev_alloc(ctx, &io.tau_prec, N * B))) return rc;
	}
	io.standalone = true;
	return SAI2B_OK;
}

// one TemplateTask call on the device: the SVD-free kernel with the generic one over the robots it declined, or the
// generic one for every robot
// the generic form of a task-level call: a robot spread over 16 lanes (a work list) or 8 (a whole batch), or — SAI2B_GENERIC_LANES=1,
// the A/B switch — the one-lane-per-robot task_kernel of rounds 1 and 2
static int launch_task_generic(sai2b_ctx* ctx, int task, const double* Np, const double* tp, double* tau_out, double* N_out, double* Ntot_out,
							   int commit_sh, int do_torque, const int* count, const int* list) {
	// (introspection: the one-lane kernel is the instantiation that fills the per-task debug outputs)
	// A whole batch stays on the one-lane kernel unless SAI2B_GENERIC_LANES asks otherwise: without the row-space chain of a
	// controller tick every JointTask behind another task takes the 7 x 7 Jacobi, and 65 536 robots through the hand-chained
	// [MFT, JT] cost 1 111 us per period with 8 lanes per robot against 692 us with one (profiles/r03_bench_task_level.txt)
	int lanes = ctx->introspection ? 0 : sai2b::generic_lanes(ctx->sw, ctx->B, count == nullptr);
	if (!count && ctx->sw.generic_lanes_env == 0) lanes = 0;
	if (lanes)
		return sai2b::launch_task_group(ctrl_params(ctx), ctx->B, lanes, task, Np, tp, tau_out, N_out, Ntot_out, commit_sh, do_torque, count, list,
										ctx->stream);
	return sai2b::launch_task(ctrl_params(ctx), ctx->B, task, Np, tp, tau_out, N_out, Ntot_out, commit_sh, do_torque, count, list, ctx->stream);
}

static int launch_task_call(sai2b_ctx* ctx, int task, const double* Np, const double* tp, double* tau_out, double* N_out, double* Ntot_out,
							int commit_sh, int do_torque) {
	const int rows = sai2b::task_cert_rows(ctx->sw, hierarchy(ctx), task, ctx->introspection);
	if (rows) {
		if (!ctx->tk.counts) {
			int rc;
			if ((rc = dev_alloc(ctx, &ctx->tk.counts, 2))) return rc;
			if ((rc = dev_alloc(ctx, &ctx->tk.list, (size_t)ctx->B))) return rc;
		}
		ctx->tk.parity ^= 1;
		if (sai2b::launch_task_cert(ctrl_params(ctx), ctx->B, task, rows, ctx->h_params.payload != nullptr, !ctx->sw.no_inlane_singular, Np, tp, tau_out, N_out, Ntot_out, commit_sh,
									do_torque, ctx->tk, ctx->stream) ||
			launch_task_generic(ctx, task, Np, tp, tau_out, N_out, Ntot_out, commit_sh, do_torque, ctx->tk.count(), ctx->tk.list))
			return set_error(ctx, SAI2B_RUNTIME_ERROR, "task launch failed");
		ctx->launches += 2;
		ctx->last_call_task = 1;
		return SAI2B_OK;
	}
	if (launch_task_generic(ctx, task, Np, tp, tau_out, N_out, Ntot_out, commit_sh, do_torque, nullptr, nullptr))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "task launch failed");
	ctx->last_call_task = 2;
	ctx->launches++;
	return SAI2B_OK;
}

extern "C" int sai2b_task_update_model(sai2b_ctx* ctx, int task, const double* N_prec, int on_device) {
	int rc = task_io(ctx, task, "sai2b_task_update_model");
	if (rc) return rc;
	sai2b_ctx::TaskIO& io = ctx->tio[task];
	io.nprec_given = N_prec != nullptr;
	if ((rc = copy_rows(ctx, io.Nprec, N_prec, N * N, on_device))) return rc;
	refresh_otg_gating(ctx);
	if ((rc = upload_params(ctx))) return rc;
	if ((rc = launch_task_call(ctx, task, io.nprec_given ? io.Nprec : nullptr, nullptr, nullptr, io.N, io.Ntot, /*commit_sh=*/1, /*do_torque=*/0)))
		return rc;
	io.model_fresh = true;
	return SAI2B_OK;
}

extern "C" int sai2b_task_compute_torques(sai2b_ctx* ctx, int task, const double* tau_prec, double* tau, int on_device) {
	int rc = task_io(ctx, task, "sai2b_task_compute_torques");
	if (rc) return rc;
	sai2b_ctx::TaskIO& io = ctx->tio[task];
	const unsigned gated = refresh_otg_gating(ctx);
	if ((rc = upload_params(ctx))) return rc;
	const double* Np = io.nprec_given ? io.Nprec : nullptr;
	const DevTask& d = ctx->h_params.task[task];
	if (d.otg_on) {	 // the task's generator advances once per torque computation, before the law
		if (((gated >> task) & 1) && !io.model_fresh) {
			// is the JointTask's range empty for this robot now (JointTask.cpp:302-306)? models of the current state, nothing committed
			if (launch_task_generic(ctx, task, Np, nullptr, nullptr, io.N, io.Ntot, 0, 0, nullptr, nullptr))
				return set_error(ctx, SAI2B_RUNTIME_ERROR, "task-range pass launch failed");
			ctx->launches++;
		}
		const int clean = ctx->goals_exposed ? 0 : (int)(~ctx->goals_dirty & ~gated & (1u << task));
		ctx->goals_dirty &= ~(1u << task);
		if (sai2b::launch_otg(ctrl_params(ctx), ctx->B, ctx->otg, clean, 1 << task, jerk_mask(ctx), ctx->stream))
			return set_error(ctx, SAI2B_RUNTIME_ERROR, "OTG launch failed");
		ctx->otg.parity ^= 1;
		ctx->launches += 2;
	}
	const double* tp = nullptr;
	if (tau_prec && on_device) {
		tp = tau_prec;
		if ((rc = caller_before_read(ctx))) return rc;
	} else if (tau_prec) {
		if ((rc = copy_rows(ctx, io.tau_prec, tau_prec, N, 0))) return rc;
		tp = io.tau_prec;
	}
	// (behind updateTaskModel of the same state the nullspaces are in place: only the torques are produced)
	if ((rc = launch_task_call(ctx, task, Np, tp, io.tau, io.model_fresh ? nullptr : io.N, io.model_fresh ? nullptr : io.Ntot, io.model_fresh ? 0 : 1, 1)))
		return rc;
	ctx->ticks += ctx->B;
	io.model_fresh = false;
	ctx->q_is_pose = true;	// computeTorques caches the task's current pose
	// a device tau_prec was read in place: the caller may overwrite it once this call has returned
	if (!tau) return (tau_prec && on_device) ? caller_after_read(ctx) : SAI2B_OK;
	if (on_device && (rc = caller_before_read(ctx))) return rc;
	HIP_TRY(ctx, hipMemcpyAsync(tau, io.tau, (size_t)N * ctx->B * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
								ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

extern "C" int sai2b_task_reinitialize(sai2b_ctx* ctx, int task) {
	if (!ctx || task < 0 || task >= ctx->T) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_task_reinitialize: bad arguments");
	if (int rc_ = flush_update(ctx)) return rc_;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = upload_params(ctx);
	if (rc) return rc;
	if (sai2b::launch_reinit(ctrl_params(ctx), ctx->B, task, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "reinit launch failed");
	if (sai2b::launch_otg_reinit(ctrl_params(ctx), ctx->B, task, 0, ctx->q, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "OTG reinit launch failed");
	ctx->goals_dirty |= 1u << task;
	ctx->goals_epoch++, ctx->otg_all_idle = false;
	ctx->launches += 2;
	ctx->models_fresh = false;
	ctx->tio[task].model_fresh = false;
	// reInitializeTask reads the pose of the current state; the other tasks keep theirs
	if (ctx->T == 1) ctx->q_is_pose = true;
	return SAI2B_OK;
}

extern "C" int sai2b_task_get_nullspaces(sai2b_ctx* ctx, int task, double* N_task, double* N_prec, double* N_total) {
	int rc = task_io(ctx, task, "sai2b_task_get_nullspaces");
	if (rc) return rc;
	sai2b_ctx::TaskIO& io = ctx->tio[task];
	if ((rc = fetch_rows(ctx, io.N, 0, N * N, N_task))) return rc;
	if ((rc = fetch_rows(ctx, io.Ntot, 0, N * N, N_total))) return rc;
	if (N_prec && !io.nprec_given) {  // identity, the value a task is constructed with (JointTask.cpp:62, MotionForceTask.cpp:138)
		const size_t B = ctx->B;
		for (int i = 0; i < N * N; i++) std::fill(N_prec + i * B, N_prec + (i + 1) * B, (i % (N + 1) == 0) ? 1.0 : 0.0);
		return SAI2B_OK;
	}
	return fetch_rows(ctx, io.Nprec, 0, N * N, N_prec);
}

extern "C" int sai2b_synchronize(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// poll for up to ~2 ms before blocking: a control loop waits for ticks of tens of microseconds, and the wake-up
	// of a blocking wait is of that order (SAI2B_BLOCKING_SYNC=1: block at once)
	if (!ctx->blocking_sync) {
		const auto t0 = std::chrono::steady_clock::now();
		for (int spin = 0;; spin++) {
			const hipError_t e = hipStreamQuery(ctx->stream);
			if (e == hipSuccess) return SAI2B_OK;
			if (e != hipErrorNotReady) break;  // let the blocking call report it
			if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
		}
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
// (a deferred model update is enqueued before the stream is handed out; a caller that keeps the handle, or a
// buffer pointer, across later sai2b_update_task_models() calls flushes with sai2b_synchronize() — INTEGRATION.md §4)
extern "C" void* sai2b_stream(sai2b_ctx* ctx) {
	if (!ctx) return nullptr;
	flush_update(ctx);
	return (void*)ctx->stream;
}
extern "C" int sai2b_set_caller_stream(sai2b_ctx* ctx, void* stream) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	ctx->caller_stream = (hipStream_t)stream;
	return SAI2B_OK;
}

extern "C" void* sai2b_device_buffer(sai2b_ctx* ctx, int which, int task) {
	if (!ctx) return nullptr;
	if (flush_update(ctx)) return nullptr;
	const bool task_ok = task >= 0 && task < ctx->T;
	switch (which) {
		case SAI2B_BUF_Q: return ctx->q;
		case SAI2B_BUF_DQ: return ctx->dq;
		case SAI2B_BUF_TAU: return ctx->tau;
		case SAI2B_BUF_GOALS:
			if (task_ok) ctx->goals_exposed = true;	 // the caller may now write goals behind the library's back
			return task_ok ? ctx->h_params.task[task].goals : nullptr;
		case SAI2B_BUF_SENSED: return task_ok ? ctx->h_params.task[task].sensed : nullptr;
		case SAI2B_BUF_STATE: return task_ok ? ctx->h_params.task[task].state : nullptr;
		case SAI2B_BUF_TASK_N: return task_ok ? ctx->tio[task].N : nullptr;
		case SAI2B_BUF_TASK_N_TOTAL: return task_ok ? ctx->tio[task].Ntot : nullptr;
		case SAI2B_BUF_PAYLOAD: return (void*)ctx->h_params.payload;
		case SAI2B_BUF_PLANT_PAYLOAD: return (void*)ctx->h_params.plant_payload;
		case SAI2B_BUF_CONTACT: return (void*)ctx->h_params.contact;
		case SAI2B_BUF_JOINT_DYNAMICS: return ctx->joint_on ? (void*)ctx->joint_rows : nullptr;
		case SAI2B_BUF_JOINT_DYNAMICS_STATE: return ctx->joint_on ? (void*)ctx->joint_status : nullptr;
		case SAI2B_BUF_EXTERNAL_WRENCH: return ctx->wrench_on ? (void*)ctx->wrench_rows : nullptr;
		case SAI2B_BUF_EXTERNAL_WRENCH_STATE: return ctx->wrench_on ? (void*)ctx->wrench_status : nullptr;
		case SAI2B_BUF_HARDWARE_ACTUATOR: return ctx->hw_on ? (void*)ctx->hw_act : nullptr;
		case SAI2B_BUF_HARDWARE_SENSOR: return ctx->hw_on ? (void*)ctx->hw_sensor : nullptr;
		case SAI2B_BUF_TAU_APPLIED: return ctx->hw_on ? (void*)ctx->hw_applied : nullptr;
		case SAI2B_BUF_Q_MEASURED: return ctx->js_on ? (void*)ctx->js_qm : nullptr;
		case SAI2B_BUF_DQ_MEASURED: return ctx->js_on ? (void*)ctx->js_dqm : nullptr;
		case SAI2B_BUF_JOINT_SENSOR: return ctx->js_on ? (void*)ctx->js_rows : nullptr;
		case SAI2B_BUF_COLLISION: return ctx->col_on && ctx->col_env_rows > 0 ? (void*)ctx->col_env : nullptr;
		case SAI2B_BUF_BODY_CONTACT: return ctx->body_on ? (void*)ctx->body_rows : nullptr;
		case SAI2B_BUF_BODY_CONTACT_STATUS: return ctx->body_on ? (void*)ctx->body_status : nullptr;
		case SAI2B_BUF_REWARD_STATE: return ctx->rew_on ? (void*)ctx->rew_state : nullptr;
		case SAI2B_BUF_REWARD_EPISODE: return ctx->rew_on ? (void*)ctx->rew_episode : nullptr;
		case SAI2B_BUF_ENV_SAMPLE: return ctx->es_on ? (void*)ctx->es_sample : nullptr;
	}
	return nullptr;
}

extern "C" int sai2b_enable_introspection(sai2b_ctx* ctx, int enable) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (enable && !ctx->h_params.dbg_M) {
		const size_t B = ctx->B;
		int rc;
		if ((rc = dev_alloc(ctx, &ctx->h_params.dbg_M, N * N * B))) return rc;
		for (int t = 0; t < ctx->T; t++) {
			DevTask& d = ctx->h_params.task[t];
			if ((rc = dev_alloc(ctx, &d.dbg_tau, N * B))) return rc;
			if ((rc = dev_alloc(ctx, &d.dbg_N, N * N * B))) return rc;
			if (d.type == SAI2B_MOTION_FORCE_TASK) {
				if ((rc = dev_alloc(ctx, &d.dbg_sigma, 8 * B))) return rc;
				if ((rc = dev_alloc(ctx, &d.dbg_J, 6 * N * B))) return rc;
				if ((rc = dev_alloc(ctx, &d.dbg_pose, 12 * B))) return rc;
				if ((rc = dev_alloc(ctx, &d.dbg_F, 12 * B))) return rc;
			}
		}
		ctx->params_dirty = true;
	}
	ctx->introspection = enable != 0;
	return SAI2B_OK;
}

static int fetch_dbg(sai2b_ctx* ctx, double* dst, const double* src, size_t rows) {
	if (!dst) return SAI2B_OK;
	if (!ctx->introspection || !src)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "introspection is not enabled: call sai2b_enable_introspection() before the tick");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	HIP_TRY(ctx, hipMemcpy(dst, src, rows * (size_t)ctx->B * sizeof(double), hipMemcpyDeviceToHost));
	return SAI2B_OK;
}

extern "C" int sai2b_get_task_nullspace(sai2b_ctx* ctx, int task, double* N_total) {
	if (!ctx || task < 0 || task >= ctx->T) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "bad task index");
	if (int rc_ = flush_update(ctx)) return rc_;
	return fetch_dbg(ctx, N_total, ctx->h_params.task[task].dbg_N, N * N);
}
extern "C" int sai2b_get_task_torques(sai2b_ctx* ctx, int task, double* tau_task) {
	if (!ctx || task < 0 || task >= ctx->T) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "bad task index");
	if (int rc_ = flush_update(ctx)) return rc_;
	return fetch_dbg(ctx, tau_task, ctx->h_params.task[task].dbg_tau, N);
}
extern "C" int sai2b_get_mft_singularity(sai2b_ctx* ctx, int task, double* sigma, double* alpha, double* ns_rank) {
	int rc = mft_task_check(ctx, task, "sai2b_get_mft_singularity");
	if (rc) return rc;
	if ((rc = flush_update(ctx))) return rc;
	const double* s = ctx->h_params.task[task].dbg_sigma;
	const size_t B = ctx->B;
	if ((rc = fetch_dbg(ctx, sigma, s, 6))) return rc;
	if ((rc = fetch_dbg(ctx, alpha, s ? s + 6 * B : nullptr, 1))) return rc;
	return fetch_dbg(ctx, ns_rank, s ? s + 7 * B : nullptr, 1);
}
// SingularityHandler members between ticks (SingularityHandler.h:211-215): how many singular directions the
// last model update found (_singularity_types.size()) and the type-1 / type-2 counters of the history
extern "C" int sai2b_get_mft_singularity_state(sai2b_ctx* ctx, int task, int* n_singular, int* type_1_count, int* type_2_count) {
	int rc = mft_task_check(ctx, task, "sai2b_get_mft_singularity_state");
	if (rc) return rc;
	if ((rc = flush_update(ctx))) return rc;
	const int* IS = ctx->h_params.task[task].istate;
	const size_t B = ctx->B;
	int* dst[3] = {n_singular, type_1_count, type_2_count};
	const int row[3] = {sai2b::IS_NTYPES, sai2b::IS_C1, sai2b::IS_C2};
	for (int k = 0; k < 3; k++)
		if (dst[k]) HIP_TRY(ctx, hipMemcpyAsync(dst[k], IS + row[k] * B, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_mft_task_forces(sai2b_ctx* ctx, int task, double* F_unit, double* F_force) {
	int rc = mft_task_check(ctx, task, "sai2b_get_mft_task_forces");
	if (rc) return rc;
	if ((rc = flush_update(ctx))) return rc;
	const double* F = ctx->h_params.task[task].dbg_F;
	if ((rc = fetch_dbg(ctx, F_unit, F, 6))) return rc;
	return fetch_dbg(ctx, F_force, F ? F + 6 * (size_t)ctx->B : nullptr, 6);
}
// rows of a device buffer to host arrays (any destination may be NULL)
static int fetch_rows(sai2b_ctx* ctx, const double* src, size_t row0, size_t rows, double* dst) {
	if (!dst) return SAI2B_OK;
	HIP_TRY(ctx, hipMemcpyAsync(dst, src + row0 * (size_t)ctx->B, rows * (size_t)ctx->B * sizeof(double), hipMemcpyDeviceToHost,
								ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
// ---- per-robot payloads ----
static int payload_target_check(sai2b_ctx* ctx, int target, const char* fn) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (target < 1 || target > 3) return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string(fn) + ": target must be SAI2B_PAYLOAD_CONTROLLER, _PLANT or _BOTH");
	return SAI2B_OK;
}
// a set changed: nothing computed from the old one may be reused
static void payload_changed(sai2b_ctx* ctx) {
	ctx->params_dirty = true;
	ctx->models_fresh = false;
	for (int t = 0; t < ctx->T; t++) ctx->tio[t].model_fresh = false;
}
extern "C" int sai2b_set_link_payload(sai2b_ctx* ctx, int target, int link, const double* mass, const double* com, const double* inertia,
									  int on_device) {
	int rc = payload_target_check(ctx, target, "sai2b_set_link_payload");
	if (rc) return rc;
	if (link < 0 || link >= N) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_link_payload: link must be in [0, dof)");
	if (!mass) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_link_payload: mass is required");
	const size_t B = ctx->B;
	if (!on_device) {
		for (size_t b = 0; b < B; b++)
			if (!std::isfinite(mass[b]) || mass[b] < 0) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_link_payload: mass must be finite and >= 0");
		for (size_t i = 0; com && i < 3 * B; i++)
			if (!std::isfinite(com[i])) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_link_payload: com must be finite");
		for (size_t i = 0; inertia && i < 6 * B; i++) {
			if (!std::isfinite(inertia[i])) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_link_payload: inertia must be finite");
			if (i < 3 * B && inertia[i] < 0) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_link_payload: ixx, iyy, izz must be >= 0");
		}
	}
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevParams& hp = ctx->h_params;
	for (int s = 0; s < 2; s++) {
		if (!(target & (1 << s))) continue;
		double*& rows = ctx->payload_rows[s];
		if (!rows && (rc = dev_alloc(ctx, &rows, (size_t)sai2b::PAYLOAD_ROWS * B))) return rc;
		if ((rc = copy_rows(ctx, rows, mass, 1, on_device))) return rc;
		if (com) {
			if ((rc = copy_rows(ctx, rows + B, com, 3, on_device))) return rc;
		} else
			HIP_TRY(ctx, hipMemsetAsync(rows + B, 0, 3 * B * sizeof(double), ctx->stream));
		if (inertia) {
			if ((rc = copy_rows(ctx, rows + 4 * B, inertia, 6, on_device))) return rc;
		} else
			HIP_TRY(ctx, hipMemsetAsync(rows + 4 * B, 0, 6 * B * sizeof(double), ctx->stream));
	}
	// both sets are written: only now does either become the one in force (a failed copy above leaves the context as it was)
	if (target & SAI2B_PAYLOAD_CONTROLLER) hp.payload = ctx->payload_rows[0], hp.payload_link = link;
	if (target & SAI2B_PAYLOAD_PLANT) hp.plant_payload = ctx->payload_rows[1], hp.plant_payload_link = link;
	payload_changed(ctx);
	return SAI2B_OK;
}
extern "C" int sai2b_clear_link_payload(sai2b_ctx* ctx, int target) {
	int rc = payload_target_check(ctx, target, "sai2b_clear_link_payload");
	if (rc) return rc;
	if ((rc = flush_update(ctx))) return rc;
	if (target & SAI2B_PAYLOAD_CONTROLLER) ctx->h_params.payload = nullptr, ctx->h_params.payload_link = 0;
	if (target & SAI2B_PAYLOAD_PLANT) ctx->h_params.plant_payload = nullptr, ctx->h_params.plant_payload_link = 0;
	payload_changed(ctx);
	return SAI2B_OK;
}
extern "C" int sai2b_get_link_payload(sai2b_ctx* ctx, int target, int* link, double* mass, double* com, double* inertia) {
	int rc = payload_target_check(ctx, target, "sai2b_get_link_payload");
	if (rc) return rc;
	if (target == SAI2B_PAYLOAD_BOTH) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_link_payload: one target at a time");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const bool plant = target == SAI2B_PAYLOAD_PLANT;
	const double* rows = plant ? ctx->h_params.plant_payload : ctx->h_params.payload;
	const size_t B = ctx->B;
	if (link) *link = rows ? (plant ? ctx->h_params.plant_payload_link : ctx->h_params.payload_link) : -1;
	if (!rows) {
		if (mass) std::fill(mass, mass + B, 0.0);
		if (com) std::fill(com, com + 3 * B, 0.0);
		if (inertia) std::fill(inertia, inertia + 6 * B, 0.0);
		return SAI2B_OK;
	}
	if ((rc = fetch_rows(ctx, rows, 0, 1, mass))) return rc;
	if ((rc = fetch_rows(ctx, rows, 1, 3, com))) return rc;
	return fetch_rows(ctx, rows, 4, 6, inertia);
}

// ---- contact in the simulated plant ----
extern "C" int sai2b_default_contact(sai2b_contact_config* cfg, int link, int n_points, const double* points) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_contact: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	cfg->link = link;
	cfg->n_points = n_points;
	cfg->friction_velocity_eps = 1e-3;
	cfg->sensor_task = -1;
	if (n_points < 1 || n_points > SAI2B_MAX_CONTACT_POINTS)
		return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_contact: n_points must be in [1, 4]");
	for (int k = 0; points && k < n_points; k++)
		for (int a = 0; a < 3; a++) cfg->points[k][a] = points[3 * k + a];
	return SAI2B_OK;
}
static std::string contact_config_error(const sai2b_contact_config* c, const sai2b_task_config* tasks, int n_tasks, int robot_dof) {
	if (!c) return "contact: null config";
	if (c->link < 0 || c->link >= robot_dof) return "contact: link must be in [0, dof)";
	if (c->n_points < 1 || c->n_points > SAI2B_MAX_CONTACT_POINTS) return "contact: n_points must be in [1, 4]";
	for (int k = 0; k < c->n_points; k++)
		for (int a = 0; a < 3; a++)
			if (!std::isfinite(c->points[k][a])) return "contact: points must be finite";
	if (!(c->friction_velocity_eps > 0) || !std::isfinite(c->friction_velocity_eps)) return "contact: friction_velocity_eps must be finite and > 0";
	if (c->sensor_task != -1 && (!tasks || c->sensor_task < 0 || c->sensor_task >= n_tasks || tasks[c->sensor_task].type != SAI2B_MOTION_FORCE_TASK))
		return "contact: sensor_task must be -1 or the index of a MotionForceTask";
	return "";
}
extern "C" int sai2b_validate_contact(const sai2b_contact_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof,
									  char* msg, int msg_len) {
	const std::string err = robot_dof == N ? contact_config_error(cfg, tasks, n_tasks, robot_dof) : "contact: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_set_contact(sai2b_ctx* ctx, const sai2b_contact_config* cfg, const double* plane_point, const double* plane_normal,
								 const double* stiffness, const double* damping, const double* friction, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	const std::string err = contact_config_error(cfg, ctx->cfg, ctx->T, N);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_" + err);
	if (!plane_point || !plane_normal || !stiffness)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_contact: plane_point, plane_normal and stiffness are required");
	const size_t B = ctx->B;
	if (!on_device) {
		for (size_t i = 0; i < 3 * B; i++)
			if (!std::isfinite(plane_point[i]) || !std::isfinite(plane_normal[i]))
				return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_contact: plane_point and plane_normal must be finite");
		for (size_t b = 0; b < B; b++) {
			const double n2 = plane_normal[b] * plane_normal[b] + plane_normal[B + b] * plane_normal[B + b] + plane_normal[2 * B + b] * plane_normal[2 * B + b];
			if (!(std::fabs(std::sqrt(n2) - 1.0) <= 1e-9))
				return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_contact: plane_normal must have unit length (within 1e-9)");
			if (!std::isfinite(stiffness[b]) || stiffness[b] < 0)
				return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_contact: stiffness must be finite and >= 0");
			if (damping && (!std::isfinite(damping[b]) || damping[b] < 0))
				return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_contact: damping must be finite and >= 0");
			if (friction && (!std::isfinite(friction[b]) || friction[b] < 0))
				return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_contact: friction must be finite and >= 0");
		}
	}
	int rc;
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevParams& hp = ctx->h_params;
	// three buffers, each created once: a failed allocation leaves the others for the next call, and no contact in force
	if (!ctx->contact_rows && (rc = dev_alloc(ctx, &ctx->contact_rows, (size_t)sai2b::CONTACT_ROWS * B))) return rc;
	if (!hp.contact_status && (rc = dev_alloc(ctx, &hp.contact_status, (size_t)sai2b::CONTACT_STATUS_ROWS * B))) return rc;
	if (!hp.contact_count && (rc = dev_alloc(ctx, &hp.contact_count, 1))) return rc;
	double* rows = ctx->contact_rows;
	if ((rc = copy_rows(ctx, rows, plane_point, 3, on_device))) return rc;
	if ((rc = copy_rows(ctx, rows + 3 * B, plane_normal, 3, on_device))) return rc;
	if ((rc = copy_rows(ctx, rows + 6 * B, stiffness, 1, on_device))) return rc;
	const double* opt[2] = {damping, friction};
	for (int k = 0; k < 2; k++) {
		if (opt[k]) {
			if ((rc = copy_rows(ctx, rows + (7 + k) * B, opt[k], 1, on_device))) return rc;
		} else
			HIP_TRY(ctx, hipMemsetAsync(rows + (7 + k) * B, 0, B * sizeof(double), ctx->stream));
	}
	// everything is written: only now does the contact become the one in force
	ctx->contact_cfg = *cfg;
	hp.contact = rows;
	hp.contact_link = cfg->link, hp.contact_n_points = cfg->n_points, hp.contact_sensor_task = cfg->sensor_task;
	std::memset(hp.contact_points, 0, sizeof(hp.contact_points));
	for (int k = 0; k < cfg->n_points; k++)
		for (int a = 0; a < 3; a++) hp.contact_points[k][a] = cfg->points[k][a];
	hp.contact_v_eps = cfg->friction_velocity_eps;
	ctx->params_dirty = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_contact(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc = flush_update(ctx)) return rc;
	// the status of the last step with a contact does not outlive it: sai2b_get_contact_state gives zeros from here on
	if (ctx->h_params.contact_status) {
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		HIP_TRY(ctx, hipMemsetAsync(ctx->h_params.contact_status, 0, (size_t)sai2b::CONTACT_STATUS_ROWS * ctx->B * sizeof(double), ctx->stream));
		HIP_TRY(ctx, hipMemsetAsync(ctx->h_params.contact_count, 0, sizeof(int), ctx->stream));
	}
	ctx->h_params.contact = nullptr;
	ctx->h_params.contact_sensor_task = -1;
	ctx->params_dirty = true;
	return SAI2B_OK;
}
extern "C" int sai2b_get_contact(sai2b_ctx* ctx, sai2b_contact_config* cfg, double* rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const bool on = ctx->h_params.contact != nullptr;
	if (cfg) {
		if (on)
			*cfg = ctx->contact_cfg;
		else {
			std::memset(cfg, 0, sizeof(*cfg));
			cfg->sensor_task = -1;
		}
	}
	if (!on) {
		if (rows) std::fill(rows, rows + (size_t)sai2b::CONTACT_ROWS * ctx->B, 0.0);
		return SAI2B_OK;
	}
	return fetch_rows(ctx, ctx->h_params.contact, 0, sai2b::CONTACT_ROWS, rows);
}
extern "C" int sai2b_get_contact_state(sai2b_ctx* ctx, double* depth, double* normal_force, double* wrench_world, int* robots_in_contact) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	const double* S = ctx->h_params.contact_status;
	if (!S) {  // never had a contact
		if (depth) std::fill(depth, depth + SAI2B_MAX_CONTACT_POINTS * B, 0.0);
		if (normal_force) std::fill(normal_force, normal_force + SAI2B_MAX_CONTACT_POINTS * B, 0.0);
		if (wrench_world) std::fill(wrench_world, wrench_world + 6 * B, 0.0);
		if (robots_in_contact) *robots_in_contact = 0;
		return SAI2B_OK;
	}
	int rc;
	if ((rc = fetch_rows(ctx, S, 0, SAI2B_MAX_CONTACT_POINTS, depth))) return rc;
	if ((rc = fetch_rows(ctx, S, SAI2B_MAX_CONTACT_POINTS, SAI2B_MAX_CONTACT_POINTS, normal_force))) return rc;
	if ((rc = fetch_rows(ctx, S, 2 * SAI2B_MAX_CONTACT_POINTS, 6, wrench_world))) return rc;
	if (robots_in_contact) {
		HIP_TRY(ctx, hipMemcpyAsync(robots_in_contact, ctx->h_params.contact_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	return SAI2B_OK;
}

// ---- joint dynamics of the simulated plant ----
extern "C" int sai2b_default_joint_dynamics(sai2b_joint_dynamics_config* cfg, int robot_dof) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_joint_dynamics: null config");
	if (robot_dof != N) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "joint dynamics: this build serves another robot size");
	std::memset(cfg, 0, sizeof(*cfg));
	for (int i = 0; i < SAI2B_MAX_DOF; i++) cfg->friction_velocity_eps[i] = 1e-2;
	return SAI2B_OK;
}
static std::string joint_dynamics_config_error(const sai2b_joint_dynamics_config* c) {
	if (!c) return "joint dynamics: null config";
	for (int i = 0; i < N; i++) {
		if (!std::isfinite(c->stop_stiffness[i]) || c->stop_stiffness[i] < 0) return "joint dynamics: stop_stiffness must be finite and >= 0";
		if (!std::isfinite(c->stop_damping[i]) || c->stop_damping[i] < 0) return "joint dynamics: stop_damping must be finite and >= 0";
		if (!std::isfinite(c->friction_velocity_eps[i]) || !(c->friction_velocity_eps[i] > 0))
			return "joint dynamics: friction_velocity_eps must be finite and > 0";
	}
	return "";
}
extern "C" int sai2b_validate_joint_dynamics(const sai2b_joint_dynamics_config* cfg, int robot_dof, char* msg, int msg_len) {
	const std::string err = robot_dof == N ? joint_dynamics_config_error(cfg) : "joint dynamics: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_sizeof_joint_dynamics_config(void) { return (int)sizeof(sai2b_joint_dynamics_config); }
extern "C" int sai2b_set_joint_dynamics(sai2b_ctx* ctx, const sai2b_joint_dynamics_config* cfg, const double* armature, const double* damping,
										const double* friction, const double* torque_limit, const double* q_lower, const double* q_upper,
										int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_joint_dynamics: null ctx");
	const std::string err = joint_dynamics_config_error(cfg);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_joint_dynamics: " + err);
	const size_t B = ctx->B, NB = (size_t)N * B;
	if (!on_device) {
		const double* nonneg[3] = {armature, damping, friction};
		const char* nonneg_name[3] = {"armature", "damping", "friction"};
		for (int k = 0; k < 3; k++)
			for (size_t i = 0; nonneg[k] && i < NB; i++)
				if (!std::isfinite(nonneg[k][i]) || nonneg[k][i] < 0)
					return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string("sai2b_set_joint_dynamics: ") + nonneg_name[k] + " must be finite and >= 0");
		for (size_t i = 0; torque_limit && i < NB; i++)
			if (!(torque_limit[i] > 0)) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_joint_dynamics: torque_limit must be > 0 (+inf: none)");
		for (size_t i = 0; i < NB; i++) {
			const double lo = q_lower ? q_lower[i] : -INFINITY, hi = q_upper ? q_upper[i] : INFINITY;
			if (std::isnan(lo) || std::isnan(hi)) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_joint_dynamics: q_lower and q_upper must not be NaN");
			if (!(lo < hi)) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_joint_dynamics: q_lower must be below q_upper");
		}
	}
	int rc;
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// three buffers, each created once: a failed allocation leaves the others for the next call, and the context as it was
	if (!ctx->joint_rows && (rc = dev_alloc(ctx, &ctx->joint_rows, (size_t)sai2b::JOINT_ROWS * NB))) return rc;
	if (!ctx->joint_status && (rc = dev_alloc(ctx, &ctx->joint_status, (size_t)sai2b::JOINT_STATUS_ROWS * NB))) return rc;
	if (!ctx->joint_counts && (rc = dev_alloc(ctx, &ctx->joint_counts, (size_t)sai2b::JOINT_COUNTS))) return rc;
	const double* src[sai2b::JOINT_ROWS] = {armature, damping, friction, torque_limit, q_lower, q_upper};
	const double neutral[sai2b::JOINT_ROWS] = {0, 0, 0, INFINITY, -INFINITY, INFINITY};
	std::vector<double> fill;
	for (int r = 0; r < sai2b::JOINT_ROWS; r++) {
		double* dst = ctx->joint_rows + (size_t)r * NB;
		if (src[r]) {
			if ((rc = copy_rows(ctx, dst, src[r], N, on_device))) return rc;
		} else if (neutral[r] == 0) {
			HIP_TRY(ctx, hipMemsetAsync(dst, 0, NB * sizeof(double), ctx->stream));
		} else {
			fill.assign(NB, neutral[r]);
			if ((rc = copy_rows(ctx, dst, fill.data(), N, 0))) return rc;
		}
	}
	// everything is written: only now do the joint dynamics become the ones in force
	ctx->joint_cfg = *cfg;
	sai2b::JointParams& J = ctx->joint;
	J.rows = ctx->joint_rows, J.status = ctx->joint_status, J.counts = ctx->joint_counts;
	for (int i = 0; i < N; i++) J.stop_k[i] = cfg->stop_stiffness[i], J.stop_c[i] = cfg->stop_damping[i], J.v_eps[i] = cfg->friction_velocity_eps[i];
	ctx->joint_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_joint_dynamics(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_joint_dynamics: null ctx");
	if (int rc = flush_update(ctx)) return rc;
	// the status of the last step with joint dynamics does not outlive them: sai2b_get_joint_dynamics_state gives zeros from here on
	if (ctx->joint_status) {
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		HIP_TRY(ctx, hipMemsetAsync(ctx->joint_status, 0, (size_t)sai2b::JOINT_STATUS_ROWS * N * ctx->B * sizeof(double), ctx->stream));
		HIP_TRY(ctx, hipMemsetAsync(ctx->joint_counts, 0, sai2b::JOINT_COUNTS * sizeof(int), ctx->stream));
	}
	ctx->joint_on = false;
	return SAI2B_OK;
}
extern "C" int sai2b_get_joint_dynamics(sai2b_ctx* ctx, sai2b_joint_dynamics_config* cfg, double* rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_joint_dynamics: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (cfg) {
		if (ctx->joint_on)
			*cfg = ctx->joint_cfg;
		else
			sai2b_default_joint_dynamics(cfg, N);
	}
	if (!ctx->joint_on) {
		const size_t NB = (size_t)N * ctx->B;
		const double neutral[sai2b::JOINT_ROWS] = {0, 0, 0, INFINITY, -INFINITY, INFINITY};
		for (int r = 0; rows && r < sai2b::JOINT_ROWS; r++) std::fill(rows + r * NB, rows + (r + 1) * NB, neutral[r]);
		return SAI2B_OK;
	}
	return fetch_rows(ctx, ctx->joint_rows, 0, (size_t)sai2b::JOINT_ROWS * N, rows);
}
extern "C" int sai2b_get_joint_dynamics_state(sai2b_ctx* ctx, double* applied_torque, double* stop_torque, double* dissipative_torque,
											  int* robots_saturated, int* robots_at_stop) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_joint_dynamics_state: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	double* dst[sai2b::JOINT_STATUS_ROWS] = {applied_torque, stop_torque, dissipative_torque};
	int* cnt[sai2b::JOINT_COUNTS] = {robots_saturated, robots_at_stop};
	const size_t NB = (size_t)N * ctx->B;
	if (!ctx->joint_status) {  // never had joint dynamics
		for (double* d : dst)
			if (d) std::fill(d, d + NB, 0.0);
		for (int* c : cnt)
			if (c) *c = 0;
		return SAI2B_OK;
	}
	int rc;
	for (int r = 0; r < sai2b::JOINT_STATUS_ROWS; r++)
		if ((rc = fetch_rows(ctx, ctx->joint_status, (size_t)r * N, N, dst[r]))) return rc;
	for (int k = 0; k < sai2b::JOINT_COUNTS; k++)
		if (cnt[k]) HIP_TRY(ctx, hipMemcpyAsync(cnt[k], ctx->joint_counts + k, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	if (robots_saturated || robots_at_stop) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

// ---- external wrench on a link of the simulated plant ----
extern "C" int sai2b_default_external_wrench(sai2b_external_wrench_config* cfg, int link) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_external_wrench: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	cfg->link = link;
	cfg->frame = SAI2B_WRENCH_WORLD;
	cfg->sensor_task = -1;
	return SAI2B_OK;
}
static std::string external_wrench_config_error(const sai2b_external_wrench_config* c, const sai2b_task_config* tasks, int n_tasks, int robot_dof) {
	if (!c) return "external wrench: null config";
	if (c->link < 0 || c->link >= robot_dof) return "external wrench: link must be in [0, dof)";
	if (c->frame != SAI2B_WRENCH_WORLD && c->frame != SAI2B_WRENCH_LINK) return "external wrench: frame must be SAI2B_WRENCH_WORLD or SAI2B_WRENCH_LINK";
	for (int a = 0; a < 3; a++)
		if (!std::isfinite(c->point[a])) return "external wrench: point must be finite";
	if (c->sensor_task != -1 && (!tasks || c->sensor_task < 0 || c->sensor_task >= n_tasks || tasks[c->sensor_task].type != SAI2B_MOTION_FORCE_TASK))
		return "external wrench: sensor_task must be -1 or the index of a MotionForceTask";
	return "";
}
extern "C" int sai2b_validate_external_wrench(const sai2b_external_wrench_config* cfg, const sai2b_task_config* tasks, int n_tasks,
											  int robot_dof, char* msg, int msg_len) {
	const std::string err =
		robot_dof == N ? external_wrench_config_error(cfg, tasks, n_tasks, robot_dof) : "external wrench: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_sizeof_external_wrench_config(void) { return (int)sizeof(sai2b_external_wrench_config); }
extern "C" int sai2b_set_external_wrench(sai2b_ctx* ctx, const sai2b_external_wrench_config* cfg, const double* force, const double* moment,
										 const double* steps, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_external_wrench: null ctx");
	const std::string err = external_wrench_config_error(cfg, ctx->cfg, ctx->T, N);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_external_wrench: " + err);
	if (!force) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_external_wrench: force is required");
	const size_t B = ctx->B;
	if (!on_device) {
		for (size_t i = 0; i < 3 * B; i++)
			if (!std::isfinite(force[i]) || (moment && !std::isfinite(moment[i])))
				return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_external_wrench: force and moment must be finite");
		for (size_t b = 0; steps && b < B; b++)
			if (std::isnan(steps[b])) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_external_wrench: steps must not be NaN");
	}
	int rc;
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// three buffers, each created once: a failed allocation leaves the others for the next call, and the context as it was
	if (!ctx->wrench_rows && (rc = dev_alloc(ctx, &ctx->wrench_rows, (size_t)sai2b::WRENCH_ROWS * B))) return rc;
	if (!ctx->wrench_status) {
		if ((rc = dev_alloc(ctx, &ctx->wrench_status, (size_t)sai2b::WRENCH_STATUS_ROWS * B))) return rc;
		HIP_TRY(ctx, hipMemsetAsync(ctx->wrench_status, 0, (size_t)sai2b::WRENCH_STATUS_ROWS * B * sizeof(double), ctx->stream));
	}
	if (!ctx->wrench_count) {
		if ((rc = dev_alloc(ctx, &ctx->wrench_count, 1))) return rc;
		HIP_TRY(ctx, hipMemsetAsync(ctx->wrench_count, 0, sizeof(int), ctx->stream));
	}
	// the rows of a wrench already in force are rewritten in place: it is taken out of force first, so that a copy that fails
	// leaves the plant without a wrench, never with rows that are half the old ones and half the new
	ctx->wrench_on = false;
	double* rows = ctx->wrench_rows;
	if ((rc = copy_rows(ctx, rows, force, 3, on_device))) return rc;
	if (moment) {
		if ((rc = copy_rows(ctx, rows + 3 * B, moment, 3, on_device))) return rc;
	} else
		HIP_TRY(ctx, hipMemsetAsync(rows + 3 * B, 0, 3 * B * sizeof(double), ctx->stream));
	if (steps) {
		if ((rc = copy_rows(ctx, rows + 6 * B, steps, 1, on_device))) return rc;
	} else {
		const std::vector<double> until_changed(B, -1.0);
		if ((rc = copy_rows(ctx, rows + 6 * B, until_changed.data(), 1, 0))) return rc;
	}
	// everything is written: only now does the wrench become the one in force (again)
	ctx->wrench_cfg = *cfg;
	sai2b::WrenchParams& W = ctx->wrench;
	W.rows = rows, W.status = ctx->wrench_status, W.count = ctx->wrench_count;
	W.link = cfg->link, W.frame = cfg->frame, W.sensor_task = cfg->sensor_task;
	for (int a = 0; a < 3; a++) W.point[a] = cfg->point[a];
	ctx->wrench_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_external_wrench(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_external_wrench: null ctx");
	if (int rc = flush_update(ctx)) return rc;
	// the status of the last step with a wrench does not outlive it: sai2b_get_external_wrench_state gives zeros from here on
	if (ctx->wrench_status) {
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		HIP_TRY(ctx, hipMemsetAsync(ctx->wrench_status, 0, (size_t)sai2b::WRENCH_STATUS_ROWS * ctx->B * sizeof(double), ctx->stream));
		HIP_TRY(ctx, hipMemsetAsync(ctx->wrench_count, 0, sizeof(int), ctx->stream));
	}
	ctx->wrench_on = false;
	return SAI2B_OK;
}
extern "C" int sai2b_get_external_wrench(sai2b_ctx* ctx, sai2b_external_wrench_config* cfg, double* rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_external_wrench: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (cfg) {
		if (ctx->wrench_on)
			*cfg = ctx->wrench_cfg;
		else
			sai2b_default_external_wrench(cfg, -1);
	}
	if (!ctx->wrench_on) {
		if (rows) std::fill(rows, rows + (size_t)sai2b::WRENCH_ROWS * ctx->B, 0.0);
		return SAI2B_OK;
	}
	return fetch_rows(ctx, ctx->wrench_rows, 0, sai2b::WRENCH_ROWS, rows);
}
extern "C" int sai2b_get_external_wrench_state(sai2b_ctx* ctx, double* wrench_world, double* torque, int* robots_pushed) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_external_wrench_state: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	if (!ctx->wrench_status || !ctx->wrench_count) {  // never had an external wrench
		if (wrench_world) std::fill(wrench_world, wrench_world + 6 * B, 0.0);
		if (torque) std::fill(torque, torque + (size_t)N * B, 0.0);
		if (robots_pushed) *robots_pushed = 0;
		return SAI2B_OK;
	}
	int rc;
	if ((rc = fetch_rows(ctx, ctx->wrench_status, 0, 6, wrench_world))) return rc;
	if ((rc = fetch_rows(ctx, ctx->wrench_status, 6, N, torque))) return rc;
	if (robots_pushed) {
		HIP_TRY(ctx, hipMemcpyAsync(robots_pushed, ctx->wrench_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	return SAI2B_OK;
}

// ---- actuator and force-sensor models ----
static_assert(sai2b::HW_MAX_DELAY == SAI2B_MAX_ACTUATION_DELAY, "sai2b_launch.h and sai2b.h disagree about the deepest torque history");
extern "C" int sai2b_default_hardware(sai2b_hardware_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_hardware: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	cfg->sensor_task = -1;
	return SAI2B_OK;
}
static std::string hardware_config_error(const sai2b_hardware_config* c, const sai2b_task_config* tasks, int n_tasks) {
	if (!c) return "hardware: null config";
	if (c->max_delay < 0 || c->max_delay > SAI2B_MAX_ACTUATION_DELAY) return "hardware: max_delay must be in [0, SAI2B_MAX_ACTUATION_DELAY]";
	if (c->sensor_task != -1 && (!tasks || c->sensor_task < 0 || c->sensor_task >= n_tasks || tasks[c->sensor_task].type != SAI2B_MOTION_FORCE_TASK))
		return "hardware: sensor_task must be -1 or the index of a MotionForceTask";
	return "";
}
// the per-robot rows given as host arrays (either may be NULL)
static std::string hardware_rows_error(const sai2b_hardware_config* c, const double* act, const double* sen, size_t B) {
	if (act) {
		for (size_t b = 0; b < B; b++) {
			const double d = act[b];
			if (!(d >= 0 && d <= c->max_delay) || d != std::floor(d)) return "hardware: the delay must be an integer in [0, max_delay]";
		}
		for (size_t i = 0; i < (size_t)N * B; i++) {
			const double alpha = act[B + i], k = act[(1 + (size_t)N) * B + i], sigma = act[(1 + 2 * (size_t)N) * B + i];
			if (!(alpha > 0 && alpha <= 1)) return "hardware: the lag coefficient alpha must be in (0, 1]";
			if (!std::isfinite(k) || k < 0) return "hardware: the gain k must be finite and not negative";
			if (!std::isfinite(sigma) || sigma < 0) return "hardware: the actuator noise sigma must be finite and not negative";
		}
	}
	if (sen) {
		for (size_t i = 0; i < 6 * B; i++) {
			if (!std::isfinite(sen[i])) return "hardware: the sensor bias must be finite";
			if (!std::isfinite(sen[6 * B + i]) || sen[6 * B + i] < 0) return "hardware: the sensor noise s must be finite and not negative";
		}
		for (size_t b = 0; b < B; b++)
			if (!(sen[12 * B + b] > 0 && sen[12 * B + b] <= 1)) return "hardware: the sensor filter coefficient alpha_s must be in (0, 1]";
	}
	return "";
}
extern "C" int sai2b_validate_hardware(const sai2b_hardware_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof, char* msg,
									   int msg_len) {
	const std::string err = robot_dof == N ? hardware_config_error(cfg, tasks, n_tasks) : "hardware: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_sizeof_hardware_config(void) { return (int)sizeof(sai2b_hardware_config); }
// the rows of the ideal signal path: d 0, alpha 1, k 1, sigma 0; beta 0, s 0, alpha_s 1
static void hardware_ideal_rows(size_t B, std::vector<double>* act, std::vector<double>* sen) {
	if (act) {
		act->assign((size_t)sai2b::HW_ACT_ROWS * B, 0.0);
		std::fill(act->begin() + B, act->begin() + (1 + 2 * (size_t)N) * B, 1.0);
	}
	if (sen) {
		sen->assign((size_t)sai2b::HW_SENSOR_ROWS * B, 0.0);
		std::fill(sen->begin() + 12 * B, sen->end(), 1.0);
	}
}
extern "C" int sai2b_set_hardware(sai2b_ctx* ctx, const sai2b_hardware_config* cfg, const double* actuator_rows, const double* sensor_rows,
								  int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_hardware: null ctx");
	std::string err = hardware_config_error(cfg, ctx->cfg, ctx->T);
	const size_t B = ctx->B;
	if (err.empty() && !on_device) err = hardware_rows_error(cfg, actuator_rows, sensor_rows, B);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_hardware: " + err);
	int rc;
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// six buffers, each created once: a failed allocation leaves the others for the next call, and the context as it was
	const size_t hist = (size_t)(SAI2B_MAX_ACTUATION_DELAY + 1) * N * B;
	if (!ctx->hw_act && (rc = dev_alloc(ctx, &ctx->hw_act, (size_t)sai2b::HW_ACT_ROWS * B))) return rc;
	if (!ctx->hw_sensor && (rc = dev_alloc(ctx, &ctx->hw_sensor, (size_t)sai2b::HW_SENSOR_ROWS * B))) return rc;
	if (!ctx->hw_history && (rc = dev_alloc(ctx, &ctx->hw_history, hist))) return rc;
	if (!ctx->hw_filter && (rc = dev_alloc(ctx, &ctx->hw_filter, (size_t)sai2b::HW_FILTER_ROWS * B))) return rc;
	if (!ctx->hw_applied && (rc = dev_alloc(ctx, &ctx->hw_applied, (size_t)N * B))) return rc;
	if (!ctx->hw_clock && (rc = dev_alloc(ctx, &ctx->hw_clock, 2 * B))) return rc;
	// rows already in force are rewritten in place: the hardware is taken out of force first, so that a copy that fails leaves
	// the context without hardware, never with rows that are half the old ones and half the new
	ctx->hw_on = false;
	// every robot starts at period 0 of episode 0; the law re-initialises the history and the filters there, zeros until then
	HIP_TRY(ctx, hipMemsetAsync(ctx->hw_clock, 0, 2 * B * sizeof(int), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->hw_history, 0, hist * sizeof(double), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->hw_filter, 0, (size_t)sai2b::HW_FILTER_ROWS * B * sizeof(double), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->hw_applied, 0, (size_t)N * B * sizeof(double), ctx->stream));
	std::vector<double> ideal_act, ideal_sen;
	hardware_ideal_rows(B, actuator_rows ? nullptr : &ideal_act, sensor_rows ? nullptr : &ideal_sen);
	if ((rc = copy_rows(ctx, ctx->hw_act, actuator_rows ? actuator_rows : ideal_act.data(), sai2b::HW_ACT_ROWS, actuator_rows ? on_device : 0)))
		return rc;
	if ((rc = copy_rows(ctx, ctx->hw_sensor, sensor_rows ? sensor_rows : ideal_sen.data(), sai2b::HW_SENSOR_ROWS, sensor_rows ? on_device : 0)))
		return rc;
	// everything is written: only now does the hardware become the one in force (again)
	ctx->hw_cfg = *cfg;
	ctx->hw_cfg.reserved = 0;
	ctx->hw_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_hardware(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_hardware: null ctx");
	if (int rc = flush_update(ctx)) return rc;
	ctx->hw_on = false;
	return SAI2B_OK;
}
extern "C" int sai2b_get_hardware(sai2b_ctx* ctx, sai2b_hardware_config* cfg, double* actuator_rows, double* sensor_rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_hardware: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (cfg) {
		if (ctx->hw_on)
			*cfg = ctx->hw_cfg;
		else
			sai2b_default_hardware(cfg);
	}
	if (!ctx->hw_on) {
		std::vector<double> act, sen;
		hardware_ideal_rows(ctx->B, actuator_rows ? &act : nullptr, sensor_rows ? &sen : nullptr);
		if (actuator_rows) std::copy(act.begin(), act.end(), actuator_rows);
		if (sensor_rows) std::copy(sen.begin(), sen.end(), sensor_rows);
		return SAI2B_OK;
	}
	if (int rc = fetch_rows(ctx, ctx->hw_act, 0, sai2b::HW_ACT_ROWS, actuator_rows)) return rc;
	return fetch_rows(ctx, ctx->hw_sensor, 0, sai2b::HW_SENSOR_ROWS, sensor_rows);
}
extern "C" int sai2b_get_hardware_state(sai2b_ctx* ctx, double* applied_torque, int* period, int* episode) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_hardware_state: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	if (!ctx->hw_on) {
		if (applied_torque) std::fill(applied_torque, applied_torque + (size_t)N * B, 0.0);
		if (period) std::fill(period, period + B, 0);
		if (episode) std::fill(episode, episode + B, 0);
		return SAI2B_OK;
	}
	if (int rc = fetch_rows(ctx, ctx->hw_applied, 0, N, applied_torque)) return rc;
	if (period) HIP_TRY(ctx, hipMemcpyAsync(period, ctx->hw_clock, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	if (episode) HIP_TRY(ctx, hipMemcpyAsync(episode, ctx->hw_clock + B, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	if (period || episode) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
// what the two stages take from the context
// ------------------------------------------------------------------------------------------------
// joint sensors (include/sai2b.h "joint sensors"; law: sai2b_joint_sensor_law.h; kernel: sai2b_joint_sensor.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int sai2b_default_joint_sensor(sai2b_joint_sensor_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_joint_sensor: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	return SAI2B_OK;
}
static std::string joint_sensor_config_error(const sai2b_joint_sensor_config* c) {
	if (!c) return "joint sensor: null config";
	if (c->max_delay < 0 || c->max_delay > SAI2B_MAX_ACTUATION_DELAY) return "joint sensor: max_delay must be in [0, SAI2B_MAX_ACTUATION_DELAY]";
	if (c->velocity_mode != 0 && c->velocity_mode != 1) return "joint sensor: velocity_mode must be 0 (tachometer) or 1 (finite difference)";
	return "";
}
static std::string joint_sensor_rows_error(const sai2b_joint_sensor_config* c, const double* rows, size_t B) {
	if (!rows) return "";
	for (size_t b = 0; b < B; b++) {
		const double d = rows[b];
		if (!(d >= 0 && d <= c->max_delay) || d != std::floor(d)) return "joint sensor: the delay must be an integer in [0, max_delay]";
	}
	for (size_t i = 0; i < (size_t)N * B; i++) {
		const double o = rows[B + i], s = rows[(1 + (size_t)N) * B + i], q = rows[(1 + 2 * (size_t)N) * B + i];
		const double r = rows[(1 + 3 * (size_t)N) * B + i], alpha = rows[(1 + 4 * (size_t)N) * B + i];
		if (!std::isfinite(o)) return "joint sensor: the offset o must be finite";
		if (!std::isfinite(s) || s < 0) return "joint sensor: the position noise s must be finite and not negative";
		if (!std::isfinite(q) || q < 0) return "joint sensor: the quantum Delta must be finite and not negative";
		if (!std::isfinite(r) || r < 0) return "joint sensor: the velocity noise r must be finite and not negative";
		if (!(alpha > 0 && alpha <= 1)) return "joint sensor: the velocity filter coefficient alpha must be in (0, 1]";
	}
	return "";
}
extern "C" int sai2b_validate_joint_sensor(const sai2b_joint_sensor_config* cfg, int robot_dof, char* msg, int msg_len) {
	const std::string err = robot_dof == N ? joint_sensor_config_error(cfg) : "joint sensor: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (err.empty()) return SAI2B_OK;
	return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_validate_joint_sensor: " + err);
}
extern "C" int sai2b_sizeof_joint_sensor_config(void) { return (int)sizeof(sai2b_joint_sensor_config); }

static void joint_sensor_ideal_rows(size_t B, std::vector<double>* rows) {
	rows->assign((size_t)sai2b::JS_ROWS * B, 0.0);
	std::fill(rows->begin() + (1 + 4 * (size_t)N) * B, rows->end(), 1.0);
}
extern "C" int sai2b_set_joint_sensor(sai2b_ctx* ctx, const sai2b_joint_sensor_config* cfg, const double* rows, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_joint_sensor: null ctx");
	std::string err = joint_sensor_config_error(cfg);
	const size_t B = ctx->B;
	if (err.empty() && !on_device) err = joint_sensor_rows_error(cfg, rows, B);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_joint_sensor: " + err);
	int rc = flush_update(ctx);
	if (rc) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t hist = (size_t)(SAI2B_MAX_ACTUATION_DELAY + 1) * 2 * N * B;
	if (!ctx->js_rows && (rc = dev_alloc(ctx, &ctx->js_rows, (size_t)sai2b::JS_ROWS * B))) return rc;
	if (!ctx->js_qm && (rc = dev_alloc(ctx, &ctx->js_qm, (size_t)N * B))) return rc;
	if (!ctx->js_dqm && (rc = dev_alloc(ctx, &ctx->js_dqm, (size_t)N * B))) return rc;
	if (!ctx->js_prev && (rc = dev_alloc(ctx, &ctx->js_prev, (size_t)N * B))) return rc;
	if (!ctx->js_filter && (rc = dev_alloc(ctx, &ctx->js_filter, (size_t)N * B))) return rc;
	if (!ctx->js_history && (rc = dev_alloc(ctx, &ctx->js_history, hist))) return rc;
	if (!ctx->js_clock && (rc = dev_alloc(ctx, &ctx->js_clock, 2 * B))) return rc;
	if (!ctx->d_params_meas && (rc = dev_alloc(ctx, &ctx->d_params_meas, 1))) return rc;
	// While q_is_pose holds, the cached pose is the controller's q: it moves to q_pose before the controller's q changes buffers.
	// A sensor already in force is taken out of force first, as sai2b_set_hardware does: a copy that fails leaves the context
	// with one view, never with rows that are half the old ones and half the new.
	if ((rc = keep_pose(ctx))) return rc;
	ctx->js_on = false;
	ctx->params_dirty = true;
	HIP_TRY(ctx, hipMemsetAsync(ctx->js_clock, 0, 2 * B * sizeof(int), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->js_history, 0, hist * sizeof(double), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->js_prev, 0, (size_t)N * B * sizeof(double), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->js_filter, 0, (size_t)N * B * sizeof(double), ctx->stream));
	std::vector<double> ideal;
	if (!rows) joint_sensor_ideal_rows(B, &ideal);
	if ((rc = copy_rows(ctx, ctx->js_rows, rows ? rows : ideal.data(), sai2b::JS_ROWS, rows ? on_device : 0))) return rc;
	ctx->js_cfg = *cfg;
	ctx->js_cfg.reserved = 0;
	ctx->js_on = true;
	// everything is written: reading 0 of every robot, episode 0
	if ((rc = joint_sensor_seed(ctx, nullptr, false))) {
		ctx->js_on = false;
		return rc;
	}
	ctx->models_fresh = false;
	for (int t = 0; t < ctx->T; t++) ctx->tio[t].model_fresh = false;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_joint_sensor(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_joint_sensor: null ctx");
	if (!ctx->js_on) return SAI2B_OK;
	int rc = flush_update(ctx);
	if (rc) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if ((rc = keep_pose(ctx))) return rc;  // the cached pose was the measured q
	ctx->js_on = false;
	ctx->params_dirty = true;
	ctx->models_fresh = false;
	for (int t = 0; t < ctx->T; t++) ctx->tio[t].model_fresh = false;
	return SAI2B_OK;
}
extern "C" int sai2b_get_joint_sensor(sai2b_ctx* ctx, sai2b_joint_sensor_config* cfg, double* rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_joint_sensor: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (cfg) {
		if (ctx->js_on)
			*cfg = ctx->js_cfg;
		else
			sai2b_default_joint_sensor(cfg);
	}
	if (!ctx->js_on) {
		if (rows) {
			std::vector<double> ideal;
			joint_sensor_ideal_rows(ctx->B, &ideal);
			std::memcpy(rows, ideal.data(), ideal.size() * sizeof(double));
		}
		return SAI2B_OK;
	}
	return fetch_rows(ctx, ctx->js_rows, 0, sai2b::JS_ROWS, rows);
}
extern "C" int sai2b_get_joint_sensor_state(sai2b_ctx* ctx, int* clock, int* episode) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_joint_sensor_state: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	if (!ctx->js_on) {
		if (clock) std::memset(clock, 0, B * sizeof(int));
		if (episode) std::memset(episode, 0, B * sizeof(int));
		return SAI2B_OK;
	}
	if (clock) HIP_TRY(ctx, hipMemcpyAsync(clock, ctx->js_clock, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	if (episode) HIP_TRY(ctx, hipMemcpyAsync(episode, ctx->js_clock + B, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_measured_state(sai2b_ctx* ctx, double* q, double* dq) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_measured_state: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = fetch_rows(ctx, ctrl_q(ctx), 0, N, q);
	if (rc) return rc;
	return fetch_rows(ctx, ctrl_dq(ctx), 0, N, dq);
}

static sai2b::HwStream hardware_stream(const sai2b_ctx* ctx) {
	sai2b::HwStream s;
	s.key0 = (unsigned)(ctx->hw_cfg.seed & 0xffffffffull), s.key1 = (unsigned)(ctx->hw_cfg.seed >> 32), s.first_robot = ctx->hw_cfg.first_robot;
	return s;
}

// ---- episode starts (the sampler of sai2b_reset_robots_sampled) ----
extern "C" int sai2b_default_reset_sampler(sai2b_reset_sampler_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_reset_sampler: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	cfg->max_tries = 8, cfg->ratio_task = -1, cfg->box_task = -1;
	return SAI2B_OK;
}
extern "C" int sai2b_validate_reset_sampler(const sai2b_reset_sampler_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof,
											char* msg, int msg_len) {
	// (whether a contact is in force is a context's business: sai2b_set_reset_sampler)
	const std::string err = robot_dof == N ? sai2b::rs_config_error(cfg, tasks, n_tasks, true) : "reset sampler: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_sizeof_reset_sampler_config(void) { return (int)sizeof(sai2b_reset_sampler_config); }
extern "C" int sai2b_reset_sampler_config_layout(const sai2b_reset_sampler_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof,
												 int block, int task, int* first_row, int* n_rows, int* total_rows) {
	if (!cfg || robot_dof != N || n_tasks < 0 || n_tasks > SAI2B_MAX_TASKS || (n_tasks > 0 && !tasks) || block < 0 || block > 4 ||
		(block == 4 && (task < 0 || task >= n_tasks)))
		return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_reset_sampler_config_layout: bad arguments");
	const sai2b::RsLayout L = sai2b::rs_layout(*cfg, tasks, n_tasks, N);
	int first = -1, rows = 0;
	if (block < 4)
		first = L.first[block], rows = N;
	else if (L.goal_first[task] >= 0)
		first = L.goal_first[task], rows = L.goal_rows[task];
	if (first_row) *first_row = first;
	if (n_rows) *n_rows = rows;
	if (total_rows) *total_rows = L.total;
	return SAI2B_OK;
}
extern "C" int sai2b_set_reset_sampler(sai2b_ctx* ctx, const sai2b_reset_sampler_config* cfg, const double* rows, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_reset_sampler: null ctx");
	std::string err = sai2b::rs_config_error(cfg, ctx->cfg, ctx->T, ctx->h_params.contact != nullptr);
	const size_t B = ctx->B;
	sai2b::RsLayout L;
	if (err.empty()) {
		L = sai2b::rs_layout(*cfg, ctx->cfg, ctx->T, N);
		if (rows && !on_device) err = sai2b::rs_rows_error(L, ctx->cfg, ctx->T, N, ctx->model.q_lower, ctx->model.q_upper, rows, B);
	}
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_reset_sampler: " + err);
	int rc;
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (ctx->rs_rows_cap < L.total) {  // (an earlier, smaller buffer stays with the context until it is destroyed)
		double* fresh = nullptr;
		if ((rc = dev_alloc(ctx, &fresh, (size_t)L.total * B))) return rc;
		ctx->rs_rows = fresh, ctx->rs_rows_cap = L.total;
	}
	if (!ctx->rs_state && (rc = dev_alloc(ctx, &ctx->rs_state, 2 * B))) return rc;
	if (!ctx->rs_counts && (rc = dev_alloc(ctx, &ctx->rs_counts, sai2b::RS_COUNTS))) return rc;
	// rows in force are rewritten in place: the sampler is taken out of force first, as sai2b_set_hardware does
	ctx->rs_on = false;
	HIP_TRY(ctx, hipMemsetAsync(ctx->rs_state, 0, 2 * B * sizeof(int), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->rs_counts, 0, sai2b::RS_COUNTS * sizeof(int), ctx->stream));
	std::vector<double> defaults;
	if (!rows) {
		defaults.resize((size_t)L.total * B);
		sai2b::rs_default_rows(L, N, ctx->model.q_lower, ctx->model.q_upper, B, defaults.data());
	}
	if ((rc = copy_rows(ctx, ctx->rs_rows, rows ? rows : defaults.data(), L.total, rows ? on_device : 0))) return rc;
	ctx->rs_cfg = *cfg;
	ctx->rs_lay = L;
	ctx->rs_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_reset_sampler(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_reset_sampler: null ctx");
	if (int rc = flush_update(ctx)) return rc;
	ctx->rs_on = false;
	return SAI2B_OK;
}
extern "C" int sai2b_get_reset_sampler(sai2b_ctx* ctx, sai2b_reset_sampler_config* cfg, double* rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_reset_sampler: null ctx");
	if (!ctx->rs_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_reset_sampler: no reset sampler is configured (sai2b_set_reset_sampler)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (cfg) *cfg = ctx->rs_cfg;
	return fetch_rows(ctx, ctx->rs_rows, 0, ctx->rs_lay.total, rows);
}
extern "C" int sai2b_get_reset_sampler_counts(sai2b_ctx* ctx, int counts[3]) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_reset_sampler_counts: null ctx");
	if (!ctx->rs_on || !counts)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_reset_sampler_counts: no reset sampler is configured (sai2b_set_reset_sampler), or counts is NULL");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->rs_counts, sai2b::RS_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_reset_sampler_state(sai2b_ctx* ctx, int* episode, int* tries) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_reset_sampler_state: null ctx");
	if (!ctx->rs_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_reset_sampler_state: no reset sampler is configured (sai2b_set_reset_sampler)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	if (episode) HIP_TRY(ctx, hipMemcpyAsync(episode, ctx->rs_state, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	if (tries) HIP_TRY(ctx, hipMemcpyAsync(tries, ctx->rs_state + B, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
// what reset_sampled_kernel takes from the context
static sai2b::RsParams reset_sampler_params(const sai2b_ctx* ctx) {
	const sai2b_reset_sampler_config& c = ctx->rs_cfg;
	sai2b::RsParams p;
	p.rows = ctx->rs_rows, p.episode = ctx->rs_state, p.tries = ctx->rs_state + ctx->B, p.counts = ctx->rs_counts;
	p.rng.key0 = (unsigned)(c.seed & 0xffffffffull), p.rng.key1 = (unsigned)(c.seed >> 32), p.rng.first_robot = c.first_robot;
	p.max_tries = c.max_tries, p.goal_tasks = c.goal_tasks, p.absolute_position = c.absolute_position;
	p.ratio_task = c.ratio_task, p.box_task = c.box_task, p.use_clearance = c.use_clearance;
	p.min_ratio = c.min_ratio, p.clearance = c.clearance;
	for (int k = 0; k < 3; k++) p.box_lower[k] = c.box_lower[k], p.box_upper[k] = c.box_upper[k];
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) p.goal_row[t] = ctx->rs_lay.goal_first[t];
	return p;
}

// ---- environment sampler (sai2b_randomize_robots) ----
extern "C" int sai2b_default_env_sampler(sai2b_env_sampler_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_env_sampler: null config");
	sai2b::env_default_config(cfg);
	return SAI2B_OK;
}
extern "C" int sai2b_validate_env_sampler(const sai2b_env_sampler_config* cfg, int robot_dof, char* msg, int msg_len) {
	const std::string err = robot_dof == N ? sai2b::env_config_error(cfg) : "env sampler: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_sizeof_env_sampler_config(void) { return (int)sizeof(sai2b_env_sampler_config); }
extern "C" int sai2b_env_sampler_config_layout(const sai2b_env_sampler_config* cfg, int robot_dof, int group, int* first_row, int* n_rows,
											   int* total_rows) {
	int g = -1;
	for (int k = 0; k < sai2b::ENV_GROUPS; k++)
		if (group == 1 << k) g = k;
	if (!cfg || robot_dof != N || g < 0) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_env_sampler_config_layout: bad arguments");
	const sai2b::EnvLayout L = sai2b::env_layout(cfg->groups & sai2b::ENV_ALL_GROUPS, N);
	if (first_row) *first_row = L.first[g];
	if (n_rows) *n_rows = L.rows[g];
	if (total_rows) *total_rows = L.total;
	return SAI2B_OK;
}
// "" or the first group of `groups` whose feature is not in force as the configuration needs it
static std::string env_feature_error(const sai2b_ctx* ctx, const sai2b_env_sampler_config& c, unsigned groups) {
	const DevParams& hp = ctx->h_params;
	if (groups & SAI2B_ENV_PAYLOAD) {
		if (!hp.plant_payload) return "SAI2B_ENV_PAYLOAD needs a plant payload (sai2b_set_link_payload)";
		if (c.payload_target == SAI2B_PAYLOAD_BOTH && (!hp.payload || hp.payload_link != hp.plant_payload_link))
			return "SAI2B_ENV_PAYLOAD with SAI2B_PAYLOAD_BOTH needs a controller payload on the plant payload's link";
	}
	if ((groups & SAI2B_ENV_CONTACT) && !hp.contact) return "SAI2B_ENV_CONTACT needs a contact (sai2b_set_contact)";
	if ((groups & SAI2B_ENV_JOINT_DYNAMICS) && !ctx->joint_on) return "SAI2B_ENV_JOINT_DYNAMICS needs joint dynamics (sai2b_set_joint_dynamics)";
	if (groups & SAI2B_ENV_HARDWARE) {
		if (!ctx->hw_on) return "SAI2B_ENV_HARDWARE needs hardware (sai2b_set_hardware)";
		if (c.delay_upper > ctx->hw_cfg.max_delay) return "delay_upper exceeds max_delay of the hardware in force";
	}
	if ((groups & SAI2B_ENV_PUSH) && !ctx->wrench_on) return "SAI2B_ENV_PUSH needs an external wrench (sai2b_set_external_wrench)";
	return "";
}
extern "C" int sai2b_set_env_sampler(sai2b_ctx* ctx, const sai2b_env_sampler_config* cfg) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_env_sampler: null ctx");
	std::string err = sai2b::env_config_error(cfg);
	if (err.empty()) err = env_feature_error(ctx, *cfg, cfg->groups);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_env_sampler: " + err);
	int rc;
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	const sai2b::EnvLayout L = sai2b::env_layout(cfg->groups, N);
	const sai2b::EnvNominal M = sai2b::env_nominal(N);
	if (!ctx->es_nominal && (rc = dev_alloc(ctx, &ctx->es_nominal, (size_t)M.total * B))) return rc;
	if (!ctx->es_sample || ctx->es_sample_cap < L.total) {	// (an earlier, smaller buffer stays with the context until it is destroyed)
		double* fresh = nullptr;
		if ((rc = dev_alloc(ctx, &fresh, (size_t)std::max(L.total, 1) * B))) return rc;
		ctx->es_sample = fresh, ctx->es_sample_cap = std::max(L.total, 1);
	}
	if (!ctx->es_counter && (rc = dev_alloc(ctx, &ctx->es_counter, B))) return rc;
	if (!ctx->es_counts && (rc = dev_alloc(ctx, &ctx->es_counts, sai2b::ENV_COUNTS))) return rc;
	// the nominal rows in force are rewritten in place: the sampler is taken out of force first, as sai2b_set_hardware does
	ctx->es_on = false;
	ctx->es_lay = L;
	HIP_TRY(ctx, hipMemsetAsync(ctx->es_counter, 0, B * sizeof(int), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->es_counts, 0, sai2b::ENV_COUNTS * sizeof(int), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->es_sample, 0, (size_t)ctx->es_sample_cap * B * sizeof(double), ctx->stream));
	auto keep = [&](int row, const double* src, int rows) {
		return hipMemcpyAsync(ctx->es_nominal + (size_t)row * B, src, (size_t)rows * B * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
	};
	const unsigned g = cfg->groups;
	if (g & SAI2B_ENV_PAYLOAD) {
		HIP_TRY(ctx, keep(M.plant_payload, ctx->payload_rows[1], sai2b::PAYLOAD_ROWS));
		if (cfg->payload_target == SAI2B_PAYLOAD_BOTH) HIP_TRY(ctx, keep(M.payload, ctx->payload_rows[0], sai2b::PAYLOAD_ROWS));
	}
	if (g & SAI2B_ENV_CONTACT) HIP_TRY(ctx, keep(M.contact, ctx->contact_rows, sai2b::CONTACT_ROWS));
	if (g & SAI2B_ENV_JOINT_DYNAMICS) HIP_TRY(ctx, keep(M.joint, ctx->joint_rows, sai2b::ENV_JOINT_PARAMS * N));
	if (g & SAI2B_ENV_HARDWARE) {
		HIP_TRY(ctx, keep(M.actuator, ctx->hw_act, sai2b::HW_ACT_ROWS));
		HIP_TRY(ctx, keep(M.sensor, ctx->hw_sensor, 12));
	}
	ctx->es_cfg = *cfg;
	ctx->es_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_env_sampler(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_env_sampler: null ctx");
	if (int rc = flush_update(ctx)) return rc;
	ctx->es_on = false;
	return SAI2B_OK;
}
extern "C" int sai2b_get_env_sampler(sai2b_ctx* ctx, sai2b_env_sampler_config* cfg) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_env_sampler: null ctx");
	if (!ctx->es_on || !cfg)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_env_sampler: no environment sampler is configured (sai2b_set_env_sampler), or cfg is NULL");
	*cfg = ctx->es_cfg;
	return SAI2B_OK;
}
extern "C" int sai2b_randomize_robots(sai2b_ctx* ctx, const unsigned char* mask, unsigned groups, int on_device) {
	const std::string fn = "sai2b_randomize_robots";
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, fn + ": null ctx");
	if (!ctx->es_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, fn + ": no environment sampler is configured (sai2b_set_env_sampler)");
	if (!mask) return set_error(ctx, SAI2B_INVALID_ARGUMENT, fn + ": mask is NULL");
	const sai2b_env_sampler_config& c = ctx->es_cfg;
	if (groups & ~c.groups) return set_error(ctx, SAI2B_INVALID_ARGUMENT, fn + ": groups names a group the sampler was not configured with");
	if (!groups) groups = c.groups;
	const std::string err = env_feature_error(ctx, c, groups);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, fn + ": " + err);
	int rc;
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	const unsigned char* d_mask = mask;
	if (on_device) {
		if ((rc = caller_before_read(ctx))) return rc;
	} else {
		if (!ctx->reset_mask && (rc = dev_alloc(ctx, &ctx->reset_mask, B))) return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->reset_mask, mask, B, hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // pageable host memory may be reused by the caller
		d_mask = ctx->reset_mask;
	}
	const sai2b::EnvNominal M = sai2b::env_nominal(N);
	sai2b::EnvParams p;
	p.groups = groups, p.both = c.payload_target == SAI2B_PAYLOAD_BOTH;
	p.counter = ctx->es_counter, p.counts = ctx->es_counts, p.sample = ctx->es_sample;
	for (int g = 0; g < sai2b::ENV_GROUPS; g++) p.sample_row[g] = ctx->es_lay.first[g];
	const double* nom = ctx->es_nominal;
	p.nom_plant_payload = nom + (size_t)M.plant_payload * B, p.nom_payload = nom + (size_t)M.payload * B;
	p.nom_contact = nom + (size_t)M.contact * B, p.nom_joint = nom + (size_t)M.joint * B;
	p.nom_actuator = nom + (size_t)M.actuator * B, p.nom_sensor = nom + (size_t)M.sensor * B;
	p.plant_payload = ctx->payload_rows[1], p.payload = ctx->payload_rows[0], p.contact = ctx->contact_rows, p.joint = ctx->joint_rows;
	p.actuator = ctx->hw_act, p.sensor = ctx->hw_sensor, p.wrench = ctx->wrench_rows;
	p.rng.key0 = (unsigned)(c.seed & 0xffffffffull), p.rng.key1 = (unsigned)(c.seed >> 32), p.rng.first_robot = c.first_robot;
	p.draw = sai2b::env_draw_params(c);
	HIP_TRY(ctx, hipMemsetAsync(ctx->es_counts, 0, sai2b::ENV_COUNTS * sizeof(int), ctx->stream));
	if (sai2b::launch_env_randomize(ctx->B, p, d_mask, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, fn + ": launch failed");
	ctx->launches++;
	if ((groups & SAI2B_ENV_PAYLOAD) && p.both) {  // the controller's model has changed: nothing computed from the old rows may be reused
		ctx->models_fresh = false;
		for (int t = 0; t < ctx->T; t++) ctx->tio[t].model_fresh = false;
	}
	return on_device ? caller_after_read(ctx) : SAI2B_OK;
}
extern "C" int sai2b_get_env_sampler_counts(sai2b_ctx* ctx, int counts[2]) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_env_sampler_counts: null ctx");
	if (!ctx->es_on || !counts)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_env_sampler_counts: no environment sampler is configured (sai2b_set_env_sampler), or counts is NULL");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->es_counts, sai2b::ENV_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_env_sampler_state(sai2b_ctx* ctx, int* draw_counter, double* sample_rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_env_sampler_state: null ctx");
	if (!ctx->es_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_env_sampler_state: no environment sampler is configured (sai2b_set_env_sampler)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	if (draw_counter) HIP_TRY(ctx, hipMemcpyAsync(draw_counter, ctx->es_counter, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	if (sample_rows && ctx->es_lay.total)
		HIP_TRY(ctx, hipMemcpyAsync(sample_rows, ctx->es_sample, (size_t)ctx->es_lay.total * B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

// ---- observations and episode-end flags ----
namespace {
constexpr int OBS_ALL_BLOCKS = SAI2B_OBS_Q | SAI2B_OBS_DQ | SAI2B_OBS_TAU | SAI2B_OBS_LIMIT_MARGIN | SAI2B_OBS_EPISODE_STEP | SAI2B_OBS_CONTACT;
constexpr int OBS_ALL_TASK_BLOCKS = SAI2B_OBS_POSE | SAI2B_OBS_TWIST | SAI2B_OBS_ERROR | SAI2B_OBS_SENSED;
constexpr int OBS_ALL_CRITERIA = (1 << SAI2B_DONE_REASONS) - 1;
constexpr int OBS_TASK_BLOCK_ROWS[sai2b::OBS_TASK_BLOCKS] = {12, 6, 8, 6};	// POSE, TWIST, ERROR, SENSED
// first rows of the global blocks and of every observed task's blocks; returns the rows of the whole observation
int observation_rows(const sai2b_observation_config& c, int row_global[sai2b::OBS_GLOBAL_BLOCKS], int row_task[SAI2B_MAX_TASKS]) {
	const int global_rows[sai2b::OBS_GLOBAL_BLOCKS] = {N, N, N, 1, 1, sai2b::CONTACT_STATUS_ROWS};
	int rows = 0;
	for (int k = 0; k < sai2b::OBS_GLOBAL_BLOCKS; k++) {
		row_global[k] = (c.blocks >> k) & 1 ? rows : -1;
		if ((c.blocks >> k) & 1) rows += global_rows[k];
	}
	int per_task = 0;
	for (int k = 0; k < sai2b::OBS_TASK_BLOCKS; k++)
		if ((c.task_blocks >> k) & 1) per_task += OBS_TASK_BLOCK_ROWS[k];
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) {
		const bool on = ((c.task_mask >> t) & 1) && per_task > 0;
		row_task[t] = on ? rows : -1;
		if (on) rows += per_task;
	}
	return rows;
}
int single_bit_index(int v, int n_bits) {
	for (int k = 0; k < n_bits; k++)
		if (v == 1 << k) return k;
	return -1;
}
std::string observation_config_error(const sai2b_observation_config* c, const sai2b_task_config* tasks, int n_tasks) {
	if (!c) return "observation: null config";
	if (c->blocks & ~OBS_ALL_BLOCKS) return "observation: unknown bits in blocks";
	if (c->task_blocks & ~OBS_ALL_TASK_BLOCKS) return "observation: unknown bits in task_blocks";
	if (c->criteria & ~OBS_ALL_CRITERIA) return "observation: unknown bits in criteria";
	const int masks[3] = {c->task_mask, c->success_task_mask, c->force_task_mask};
	const char* mask_name[3] = {"task_mask", "success_task_mask", "force_task_mask"};
	for (int m = 0; m < 3; m++)
		for (int t = 0; t < 32; t++)
			if (((unsigned)masks[m] >> t) & 1u)
				if (!tasks || t >= n_tasks || t >= SAI2B_MAX_TASKS || tasks[t].type != SAI2B_MOTION_FORCE_TASK)
					return std::string("observation: ") + mask_name[m] + " selects a task that is not a MotionForceTask";
	const double thr[4] = {c->pos_tolerance, c->ori_tolerance, c->joint_limit_margin, c->max_sensed_force};
	for (double v : thr)
		if (!std::isfinite(v) || v < 0) return "observation: thresholds must be finite and >= 0";
	for (int i = 0; i < N; i++)
		if (!std::isfinite(c->max_joint_speed[i]) || c->max_joint_speed[i] < 0) return "observation: max_joint_speed must be finite and >= 0";
	if (c->max_episode_steps < 0) return "observation: max_episode_steps must be >= 0";
	if ((c->criteria & SAI2B_DONE_TIMEOUT) && c->max_episode_steps < 1) return "observation: TIMEOUT needs max_episode_steps >= 1";
	if ((c->criteria & SAI2B_DONE_SUCCESS) && !c->success_task_mask) return "observation: SUCCESS needs a task in success_task_mask";
	if ((c->criteria & SAI2B_DONE_FORCE) && !c->force_task_mask) return "observation: FORCE needs a task in force_task_mask";
	return "";
}
}  // namespace
extern "C" int sai2b_default_observation(sai2b_observation_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_observation: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	return SAI2B_OK;
}
extern "C" int sai2b_sizeof_observation_config(void) { return (int)sizeof(sai2b_observation_config); }
extern "C" int sai2b_validate_observation(const sai2b_observation_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof,
										  char* msg, int msg_len) {
	const std::string err = robot_dof == N ? observation_config_error(cfg, tasks, n_tasks) : "observation: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_observation_config_layout(const sai2b_observation_config* cfg, int robot_dof, int block, int task, int* first_row,
											   int* n_rows, int* total_rows) {
	if (!cfg || robot_dof != N) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_observation_config_layout: bad arguments");
	const int k = single_bit_index(block, task < 0 ? sai2b::OBS_GLOBAL_BLOCKS : sai2b::OBS_TASK_BLOCKS);
	if (k < 0 || task < -1 || task >= SAI2B_MAX_TASKS)
		return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_observation_config_layout: block must be one known flag and task -1 or a task index");
	int row_global[sai2b::OBS_GLOBAL_BLOCKS], row_task[SAI2B_MAX_TASKS];
	const int rows = observation_rows(*cfg, row_global, row_task);
	int first = -1, n = 0;
	if (task < 0) {
		const int global_rows[sai2b::OBS_GLOBAL_BLOCKS] = {N, N, N, 1, 1, sai2b::CONTACT_STATUS_ROWS};
		if (row_global[k] >= 0) first = row_global[k], n = global_rows[k];
	} else if (row_task[task] >= 0 && ((cfg->task_blocks >> k) & 1)) {
		first = row_task[task], n = OBS_TASK_BLOCK_ROWS[k];
		for (int j = 0; j < k; j++)
			if ((cfg->task_blocks >> j) & 1) first += OBS_TASK_BLOCK_ROWS[j];
	}
	if (first_row) *first_row = first;
	if (n_rows) *n_rows = n;
	if (total_rows) *total_rows = rows;
	return SAI2B_OK;
}
extern "C" int sai2b_set_observation(sai2b_ctx* ctx, const sai2b_observation_config* cfg) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_observation: null ctx");
	const std::string err = observation_config_error(cfg, ctx->cfg, ctx->T);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_" + err);
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc;
	const size_t B = ctx->B;
	if (!ctx->obs_steps && (rc = dev_alloc(ctx, &ctx->obs_steps, B))) return rc;
	// (the reward's two counters stand behind the seven of the observation, so that sai2b_observe_reward zeroes all with one memset)
	if (!ctx->obs_counts && (rc = dev_alloc(ctx, &ctx->obs_counts, (size_t)sai2b::OBS_COUNTS + sai2b::REW_COUNTS))) return rc;
	// a new configuration starts every robot's episode (stream-ordered behind observes already enqueued)
	HIP_TRY(ctx, hipMemsetAsync(ctx->obs_steps, 0, B * sizeof(int), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->obs_counts, 0, (sai2b::OBS_COUNTS + sai2b::REW_COUNTS) * sizeof(int), ctx->stream));
	sai2b::ObsParams o;
	o.blocks = cfg->blocks, o.task_mask = cfg->task_mask, o.task_blocks = cfg->task_blocks;
	o.criteria = cfg->criteria, o.success_mask = cfg->success_task_mask, o.force_mask = cfg->force_task_mask;
	o.max_steps = cfg->max_episode_steps;
	o.pos_tol = cfg->pos_tolerance, o.ori_tol = cfg->ori_tolerance, o.limit_margin = cfg->joint_limit_margin, o.max_force = cfg->max_sensed_force;
	for (int i = 0; i < N; i++) o.max_speed[i] = cfg->max_joint_speed[i];
	ctx->obs_rows = observation_rows(*cfg, o.row_global, o.row_task);
	ctx->obs = o;
	ctx->obs_cfg = *cfg;
	ctx->obs_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_observation(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_observation: null ctx");
	ctx->obs_on = false;
	ctx->obs_rows = 0;
	return SAI2B_OK;
}
extern "C" int sai2b_observation_rows(sai2b_ctx* ctx) { return ctx && ctx->obs_on ? ctx->obs_rows : -1; }
extern "C" int sai2b_observation_layout(sai2b_ctx* ctx, int block, int task, int* first_row, int* n_rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_observation_layout: null ctx");
	if (!ctx->obs_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_observation_layout: no observation is configured (sai2b_set_observation)");
	const int rc = sai2b_observation_config_layout(&ctx->obs_cfg, N, block, task, first_row, n_rows, nullptr);
	return rc ? set_error(ctx, rc, g_error) : SAI2B_OK;
}
extern "C" int sai2b_observe(sai2b_ctx* ctx, double* out, unsigned char* done, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_observe: null ctx");
	if (!ctx->obs_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_observe: no observation is configured (sai2b_set_observation)");
	int rc = flush_update(ctx);	 // a deferred model update happens before anything is observed
	if (rc) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if ((rc = upload_params(ctx))) return rc;
	const size_t B = ctx->B;
	const bool want_out = out && ctx->obs_rows > 0;
	double* d_out = want_out ? out : nullptr;
	unsigned char* d_done = done;
	if (on_device) {
		// device results are written on the ctx stream: what the caller's stream still does with those buffers comes first
		if ((want_out || done) && (rc = caller_before_read(ctx))) return rc;
	} else {
		if (want_out) {
			if (ctx->obs_out_rows < ctx->obs_rows) {  // a configuration with more rows: the smaller staging buffer goes
				if (ctx->obs_out) {
					HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), (void*)ctx->obs_out), ctx->allocs.end());
					HIP_TRY(ctx, hipFree(ctx->obs_out));
					ctx->obs_out = nullptr, ctx->obs_out_rows = 0;
				}
				if ((rc = dev_alloc(ctx, &ctx->obs_out, (size_t)ctx->obs_rows * B))) return rc;
				ctx->obs_out_rows = ctx->obs_rows;
			}
			d_out = ctx->obs_out;
		}
		if (done) {
			if (!ctx->obs_done && (rc = dev_alloc(ctx, &ctx->obs_done, B))) return rc;
			d_done = ctx->obs_done;
		}
	}
	HIP_TRY(ctx, hipMemsetAsync(ctx->obs_counts, 0, sai2b::OBS_COUNTS * sizeof(int), ctx->stream));
	if (sai2b::launch_observe(ctrl_params(ctx), ctx->B, ctx->obs, d_out, d_done, ctx->obs_steps, ctx->obs_counts, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "sai2b_observe: launch failed");
	ctx->launches++;
	if (on_device) return (want_out || done) ? caller_after_read(ctx) : SAI2B_OK;
	if (want_out) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)ctx->obs_rows * B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (done) HIP_TRY(ctx, hipMemcpyAsync(done, d_done, B, hipMemcpyDeviceToHost, ctx->stream));
	if (want_out || done) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_done_counts(sai2b_ctx* ctx, int counts[7]) {
	if (!ctx || !counts) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_done_counts: bad arguments");
	if (!ctx->obs_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_done_counts: no observation is configured (sai2b_set_observation)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->obs_counts, sai2b::OBS_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

// ---- rewards and episode returns ----
namespace {
constexpr int REW_ALL_TERMS = (1 << SAI2B_REWARD_TERMS) - 1, REW_ALL_TASK_TERMS = (1 << SAI2B_REWARD_TASK_TERMS) - 1;
// rows of the global terms and of every task's terms; returns the rows of all terms
int reward_rows(const sai2b_reward_config& c, int row_global[SAI2B_REWARD_TERMS], int row_task[SAI2B_MAX_TASKS], int off_task[SAI2B_REWARD_TASK_TERMS]) {
	int rows = 0;
	for (int k = 0; k < SAI2B_REWARD_TERMS; k++) row_global[k] = (c.terms >> k) & 1 ? rows++ : -1;
	int per_task = 0;
	for (int k = 0; k < SAI2B_REWARD_TASK_TERMS; k++) off_task[k] = (c.task_terms >> k) & 1 ? per_task++ : -1;
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) {
		const bool on = ((c.task_mask >> t) & 1) && per_task > 0;
		row_task[t] = on ? rows : -1;
		if (on) rows += per_task;
	}
	return rows;
}
std::string reward_config_error(const sai2b_reward_config* c, const sai2b_task_config* tasks, int n_tasks) {
	if (!c) return "reward: null config";
	if (c->terms & ~REW_ALL_TERMS) return "reward: unknown bits in terms";
	if (c->task_terms & ~REW_ALL_TASK_TERMS) return "reward: unknown bits in task_terms";
	for (int t = 0; t < 32; t++)
		if (((unsigned)c->task_mask >> t) & 1u)
			if (!tasks || t >= n_tasks || t >= SAI2B_MAX_TASKS || tasks[t].type != SAI2B_MOTION_FORCE_TASK)
				return "reward: task_mask selects a task that is not a MotionForceTask";
	if (c->task_terms && !c->task_mask) return "reward: task_terms needs a task in task_mask";
	if (c->task_mask && !c->task_terms) return "reward: task_mask needs a term in task_terms";
	for (double v : c->weight)
		if (!std::isfinite(v)) return "reward: weights must be finite";
	for (int t = 0; t < SAI2B_MAX_TASKS; t++)
		for (double v : c->task_weight[t])
			if (!std::isfinite(v)) return "reward: weights must be finite";
	for (double v : c->done_value)
		if (!std::isfinite(v)) return "reward: done_value must be finite";
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) {
		if (!std::isfinite(c->pos_scale[t]) || !std::isfinite(c->ori_scale[t])) return "reward: scales must be finite";
		const bool on = (c->task_mask >> t) & 1;
		if (on && (c->task_terms & SAI2B_REW_POS_TANH) && !(c->pos_scale[t] > 0)) return "reward: POS_TANH needs pos_scale > 0";
		if (on && (c->task_terms & SAI2B_REW_ORI_TANH) && !(c->ori_scale[t] > 0)) return "reward: ORI_TANH needs ori_scale > 0";
		if (!std::isfinite(c->force_soft_limit[t]) || c->force_soft_limit[t] < 0) return "reward: force_soft_limit must be finite and >= 0";
	}
	if (!std::isfinite(c->limit_soft_margin) || c->limit_soft_margin < 0) return "reward: limit_soft_margin must be finite and >= 0";
	if (!(c->gamma >= 0 && c->gamma <= 1)) return "reward: gamma must be in [0, 1]";
	if (!std::isfinite(c->nonfinite_reward)) return "reward: nonfinite_reward must be finite";
	if (!c->terms && !c->task_terms) return "reward: no term is selected";
	return "";
}
}  // namespace
extern "C" int sai2b_default_reward(sai2b_reward_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_reward: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) cfg->pos_scale[t] = cfg->ori_scale[t] = 1.0;
	cfg->gamma = 1.0;
	return SAI2B_OK;
}
extern "C" int sai2b_sizeof_reward_config(void) { return (int)sizeof(sai2b_reward_config); }
extern "C" int sai2b_validate_reward(const sai2b_reward_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof, char* msg,
									 int msg_len) {
	const std::string err = robot_dof == N ? reward_config_error(cfg, tasks, n_tasks) : "reward: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_reward_config_layout(const sai2b_reward_config* cfg, int term, int task, int* first_row, int* n_rows, int* total_rows) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_reward_config_layout: bad arguments");
	const int k = single_bit_index(term, task < 0 ? SAI2B_REWARD_TERMS : SAI2B_REWARD_TASK_TERMS);
	if (k < 0 || task < -1 || task >= SAI2B_MAX_TASKS)
		return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_reward_config_layout: term must be one known flag and task -1 or a task index");
	int row_global[SAI2B_REWARD_TERMS], row_task[SAI2B_MAX_TASKS], off_task[SAI2B_REWARD_TASK_TERMS];
	const int rows = reward_rows(*cfg, row_global, row_task, off_task);
	int first = -1;
	if (task < 0)
		first = row_global[k];
	else if (row_task[task] >= 0 && off_task[k] >= 0)
		first = row_task[task] + off_task[k];
	if (first_row) *first_row = first;
	if (n_rows) *n_rows = first >= 0 ? 1 : 0;
	if (total_rows) *total_rows = rows;
	return SAI2B_OK;
}
// every robot's accumulators at their start values, stream-ordered
static int reward_state_start(sai2b_ctx* ctx) {
	const size_t B = ctx->B;
	HIP_TRY(ctx, hipMemsetAsync(ctx->rew_state, 0, (size_t)sai2b::REW_STATE_ROWS * B * sizeof(double), ctx->stream));
	HIP_TRY(ctx, hipMemsetAsync(ctx->rew_episode, 0, (size_t)sai2b::REW_EPISODE_ROWS * B * sizeof(int), ctx->stream));
	const std::vector<double> ones(B, 1.0);
	HIP_TRY(ctx, hipMemcpyAsync(ctx->rew_state + (size_t)sai2b::REW_DISC * B, ones.data(), B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // `ones` goes out of scope
	return SAI2B_OK;
}
extern "C" int sai2b_set_reward(sai2b_ctx* ctx, const sai2b_reward_config* cfg) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_reward: null ctx");
	const std::string err = reward_config_error(cfg, ctx->cfg, ctx->T);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_" + err);
	if (!ctx->obs_on)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_reward: no observation is configured (sai2b_set_observation): the done criteria live there");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc;
	const size_t B = ctx->B;
	if (!ctx->rew_state && (rc = dev_alloc(ctx, &ctx->rew_state, (size_t)sai2b::REW_STATE_ROWS * B))) return rc;
	if (!ctx->rew_episode && (rc = dev_alloc(ctx, &ctx->rew_episode, (size_t)sai2b::REW_EPISODE_ROWS * B))) return rc;
	ctx->rew_counts = ctx->obs_counts + sai2b::OBS_COUNTS;	// allocated with the observation's counters (sai2b_set_observation)
	if ((rc = reward_state_start(ctx))) return rc;
	HIP_TRY(ctx, hipMemsetAsync(ctx->rew_counts, 0, sai2b::REW_COUNTS * sizeof(int), ctx->stream));
	sai2b::RewParams w;
	w.terms = cfg->terms, w.task_mask = cfg->task_terms ? cfg->task_mask : 0, w.task_terms = cfg->task_terms;
	ctx->rew_rows = reward_rows(*cfg, w.row_global, w.row_task, w.off_task);
	for (int k = 0; k < SAI2B_REWARD_TERMS; k++) w.global_rows += (cfg->terms >> k) & 1;
	w.task_rows = ctx->rew_rows - w.global_rows;
	for (int k = 0; k < SAI2B_REWARD_TERMS; k++) w.weight[k] = cfg->weight[k];
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) {
		w.pos_scale[t] = cfg->pos_scale[t], w.ori_scale[t] = cfg->ori_scale[t], w.force_soft_limit[t] = cfg->force_soft_limit[t];
		if (w.row_task[t] < 0) continue;
		for (int k = 0; k < SAI2B_REWARD_TASK_TERMS; k++)
			if (w.off_task[k] >= 0) w.row_weight[w.row_task[t] - w.global_rows + w.off_task[k]] = cfg->task_weight[t][k];
	}
	for (int r = 0; r < SAI2B_DONE_REASONS; r++) w.done_value[r] = cfg->done_value[r];
	w.limit_soft_margin = cfg->limit_soft_margin, w.gamma = cfg->gamma, w.nonfinite_reward = cfg->nonfinite_reward;
	w.state = ctx->rew_state, w.episode = ctx->rew_episode, w.counts = ctx->rew_counts;
	ctx->rew = w;
	ctx->rew_cfg = *cfg;
	ctx->rew_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_reward(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_reward: null ctx");
	ctx->rew_on = false;
	ctx->rew_rows = 0;
	return SAI2B_OK;
}
extern "C" int sai2b_reward_rows(sai2b_ctx* ctx) { return ctx && ctx->rew_on ? ctx->rew_rows : -1; }
extern "C" int sai2b_reward_layout(sai2b_ctx* ctx, int term, int task, int* first_row, int* n_rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_reward_layout: null ctx");
	if (!ctx->rew_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_reward_layout: no reward is configured (sai2b_set_reward)");
	const int rc = sai2b_reward_config_layout(&ctx->rew_cfg, term, task, first_row, n_rows, nullptr);
	return rc ? set_error(ctx, rc, g_error) : SAI2B_OK;
}
extern "C" int sai2b_observe_reward(sai2b_ctx* ctx, double* out, unsigned char* done, double* reward, double* terms, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_observe_reward: null ctx");
	if (!ctx->obs_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_observe_reward: no observation is configured (sai2b_set_observation)");
	if (!ctx->rew_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_observe_reward: no reward is configured (sai2b_set_reward)");
	int rc = flush_update(ctx);	 // a deferred model update happens before anything is observed
	if (rc) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if ((rc = upload_params(ctx))) return rc;
	const size_t B = ctx->B;
	const bool want_out = out && ctx->obs_rows > 0;
	const bool any = want_out || done || reward || terms;
	double* d_out = want_out ? out : nullptr;
	unsigned char* d_done = done;
	sai2b::RewParams w = ctx->rew;
	w.reward = reward, w.rows = terms;
	if (on_device) {
		// device results are written on the ctx stream: what the caller's stream still does with those buffers comes first
		if (any && (rc = caller_before_read(ctx))) return rc;
	} else {
		if (want_out) {
			if (ctx->obs_out_rows < ctx->obs_rows) {  // a configuration with more rows: the smaller staging buffer goes
				if (ctx->obs_out) {
					HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), (void*)ctx->obs_out), ctx->allocs.end());
					HIP_TRY(ctx, hipFree(ctx->obs_out));
					ctx->obs_out = nullptr, ctx->obs_out_rows = 0;
				}
				if ((rc = dev_alloc(ctx, &ctx->obs_out, (size_t)ctx->obs_rows * B))) return rc;
				ctx->obs_out_rows = ctx->obs_rows;
			}
			d_out = ctx->obs_out;
		}
		if (done) {
			if (!ctx->obs_done && (rc = dev_alloc(ctx, &ctx->obs_done, B))) return rc;
			d_done = ctx->obs_done;
		}
		if (reward || terms) {	// one staging buffer for both, sized for every term of any configuration
			const size_t max_rows = 1 + SAI2B_REWARD_TERMS + SAI2B_MAX_TASKS * SAI2B_REWARD_TASK_TERMS;
			if (!ctx->rew_out && (rc = dev_alloc(ctx, &ctx->rew_out, max_rows * B))) return rc;
			if (reward) w.reward = ctx->rew_out;
			if (terms) w.rows = ctx->rew_out + B;
		}
	}
	HIP_TRY(ctx, hipMemsetAsync(ctx->obs_counts, 0, (sai2b::OBS_COUNTS + sai2b::REW_COUNTS) * sizeof(int), ctx->stream));
	if (sai2b::launch_observe_reward(ctrl_params(ctx), ctx->B, ctx->obs, w, d_out, d_done, ctx->obs_steps, ctx->obs_counts, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "sai2b_observe_reward: launch failed");
	ctx->launches++;
	if (on_device) return any ? caller_after_read(ctx) : SAI2B_OK;
	if (want_out) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)ctx->obs_rows * B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (done) HIP_TRY(ctx, hipMemcpyAsync(done, d_done, B, hipMemcpyDeviceToHost, ctx->stream));
	if (reward) HIP_TRY(ctx, hipMemcpyAsync(reward, w.reward, B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (terms) HIP_TRY(ctx, hipMemcpyAsync(terms, w.rows, (size_t)ctx->rew_rows * B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (any) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_reward_counts(sai2b_ctx* ctx, int counts[2]) {
	if (!ctx || !counts) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_reward_counts: bad arguments");
	if (!ctx->rew_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_reward_counts: no reward is configured (sai2b_set_reward)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->rew_counts, sai2b::REW_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_episode_stats(sai2b_ctx* ctx, double* ret, double* discount, double* last_return, int* last_length) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_episode_stats: null ctx");
	if (!ctx->rew_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_episode_stats: no reward is configured (sai2b_set_reward)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	double* dst[3] = {ret, discount, last_return};
	for (int k = 0; k < 3; k++)
		if (dst[k]) HIP_TRY(ctx, hipMemcpyAsync(dst[k], ctx->rew_state + k * B, B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (last_length) HIP_TRY(ctx, hipMemcpyAsync(last_length, ctx->rew_episode, B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

// ------------------------------------------------------------------------------------------------
// collision proximity (include/sai2b.h "collision proximity"; law: sai2b_collision_law.h; kernels: sai2b_collision.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int sai2b_default_collision(sai2b_collision_config* cfg, int n_spheres, const int* link, const double* centre, const double* radius) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_collision: null config");
	if (n_spheres < 1 || n_spheres > SAI2B_MAX_COLLISION_SPHERES)
		return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_collision: n_spheres must be in [1, SAI2B_MAX_COLLISION_SPHERES]");
	if (!link || !centre || !radius) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_collision: link, centre and radius are required");
	std::memset(cfg, 0, sizeof(*cfg));
	cfg->n_spheres = n_spheres;
	cfg->blocks = SAI2B_COL_DISTANCE;
	for (int k = 0; k < n_spheres; k++) {
		cfg->link[k] = link[k];
		for (int a = 0; a < 3; a++) cfg->centre[k][a] = centre[3 * k + a];
		cfg->radius[k] = radius[k];
		if (link[k] >= 0) cfg->env_mask |= 1u << k;
	}
	for (int i = 0; i < n_spheres; i++)
		for (int j = i + 1; j < n_spheres; j++)
			if (std::abs(link[i] - link[j]) >= 2) cfg->pair_mask[i] |= 1u << j;
	return SAI2B_OK;
}
static std::string collision_config_error(const sai2b_collision_config* c) {
	if (!c) return "collision: null config";
	if (c->n_spheres < 1 || c->n_spheres > SAI2B_MAX_COLLISION_SPHERES) return "collision: n_spheres must be in [1, SAI2B_MAX_COLLISION_SPHERES]";
	if (c->n_planes < 0 || c->n_planes > SAI2B_MAX_COLLISION_PLANES) return "collision: n_planes must be in [0, SAI2B_MAX_COLLISION_PLANES]";
	if (c->n_obstacles < 0 || c->n_obstacles > SAI2B_MAX_COLLISION_OBSTACLES) return "collision: n_obstacles must be in [0, SAI2B_MAX_COLLISION_OBSTACLES]";
	const unsigned beyond = c->n_spheres == 32 ? 0u : ~((1u << c->n_spheres) - 1u);
	for (int k = 0; k < c->n_spheres; k++) {
		if (c->link[k] < -1 || c->link[k] >= N) return "collision: a sphere's link must be in [-1, dof)";
		for (int a = 0; a < 3; a++)
			if (!std::isfinite(c->centre[k][a])) return "collision: a sphere's centre must be finite";
		if (!std::isfinite(c->radius[k]) || c->radius[k] < 0) return "collision: a sphere's radius must be finite and not negative";
	}
	if (c->env_mask & beyond) return "collision: env_mask has bits beyond n_spheres";
	for (int i = 0; i < SAI2B_MAX_COLLISION_SPHERES; i++) {
		if (i >= c->n_spheres && c->pair_mask[i]) return "collision: pair_mask has entries beyond n_spheres";
		if (c->pair_mask[i] & beyond) return "collision: pair_mask has bits beyond n_spheres";
		if (c->pair_mask[i] & ((2u << i) - 1u)) return "collision: a pair (i, j) needs i < j";
	}
	if (c->blocks & ~sai2b::COL_ALL_BLOCKS) return "collision: unknown bits in blocks";
	if (!std::isfinite(c->margin_plane) || !std::isfinite(c->margin_obstacle) || !std::isfinite(c->margin_self)) return "collision: the margins must be finite";
	if (c->view != 0 && c->view != 1) return "collision: view must be 0 (the plant's q) or 1 (the measured q)";
	return "";
}
// host rows: a plane or an obstacle with a NaN is absent; the others are held to what the law assumes
static std::string collision_rows_error(const sai2b_collision_config* c, const double* rows, size_t B) {
	if (!rows) return "";
	for (int p = 0; p < c->n_planes; p++) {
		const double* r = rows + (size_t)sai2b::COL_PLANE_ROWS * p * B;
		for (size_t b = 0; b < B; b++) {
			bool absent = false, inf = false;
			for (int a = 0; a < 6; a++) absent = absent || std::isnan(r[a * B + b]), inf = inf || std::isinf(r[a * B + b]);
			if (absent) continue;
			if (inf) return "collision: a plane's rows must be finite (or hold a NaN: absent)";
			const double n2 = r[3 * B + b] * r[3 * B + b] + r[4 * B + b] * r[4 * B + b] + r[5 * B + b] * r[5 * B + b];
			if (!(std::fabs(std::sqrt(n2) - 1.0) <= 1e-9)) return "collision: a plane's normal must have unit length (within 1e-9)";
		}
	}
	for (int o = 0; o < c->n_obstacles; o++) {
		const double* r = rows + ((size_t)sai2b::COL_PLANE_ROWS * c->n_planes + (size_t)sai2b::COL_OBSTACLE_ROWS * o) * B;
		for (size_t b = 0; b < B; b++) {
			bool absent = false, inf = false;
			for (int a = 0; a < 4; a++) absent = absent || std::isnan(r[a * B + b]), inf = inf || std::isinf(r[a * B + b]);
			if (absent) continue;
			if (inf) return "collision: an obstacle's rows must be finite (or hold a NaN: absent)";
			if (r[3 * B + b] < 0) return "collision: an obstacle's radius must not be negative";
		}
	}
	return "";
}
extern "C" int sai2b_validate_collision(const sai2b_collision_config* cfg, int robot_dof, char* msg, int msg_len) {
	const std::string err = robot_dof == N ? collision_config_error(cfg) : "collision: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (err.empty()) return SAI2B_OK;
	return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_validate_collision: " + err);
}
extern "C" int sai2b_sizeof_collision_config(void) { return (int)sizeof(sai2b_collision_config); }
extern "C" int sai2b_collision_config_layout(const sai2b_collision_config* cfg, int robot_dof, int block, int category, int* first_row,
											 int* n_rows, int* total_rows, int* env_rows) {
	if (robot_dof != N) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_collision_config_layout: this build serves another robot size");
	const std::string err = collision_config_error(cfg);
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_collision_config_layout: " + err);
	int k = -1;
	for (int i = 0; i < sai2b::COL_BLOCKS; i++)
		if (block == (1 << i)) k = i;
	if (k < 0) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_collision_config_layout: block must be exactly one SAI2B_COL_* flag");
	if (category < -1 || category >= sai2b::COL_CATEGORIES || (category >= 0 && block == SAI2B_COL_CENTRES))
		return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_collision_config_layout: category must be -1, or 0..2 for a per-category block");
	int row[sai2b::COL_BLOCKS];
	const int rows = sai2b::col_layout(cfg->blocks, N, cfg->n_spheres, row);
	int first = row[k], n = first < 0 ? 0 : sai2b::col_block_rows(block, N, cfg->n_spheres);
	if (first >= 0 && category >= 0) n /= sai2b::COL_CATEGORIES, first += n * category;
	if (first_row) *first_row = first;
	if (n_rows) *n_rows = n;
	if (total_rows) *total_rows = rows;
	if (env_rows) *env_rows = sai2b::col_env_rows(cfg->n_planes, cfg->n_obstacles);
	return SAI2B_OK;
}
static int collision_counts_alloc(sai2b_ctx* ctx) {
	if (ctx->col_counts) return SAI2B_OK;
	if (int rc = dev_alloc(ctx, &ctx->col_counts, (size_t)sai2b::COL_COUNTS + 1)) return rc;
	HIP_TRY(ctx, hipMemsetAsync(ctx->col_counts, 0, (sai2b::COL_COUNTS + 1) * sizeof(int), ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_set_collision(sai2b_ctx* ctx, const sai2b_collision_config* cfg, const double* rows, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_collision: null ctx");
	std::string err = collision_config_error(cfg);
	const size_t B = ctx->B;
	if (err.empty() && !on_device) err = collision_rows_error(cfg, rows, B);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_" + err);
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc;
	if (!ctx->col_env && (rc = dev_alloc(ctx, &ctx->col_env, (size_t)sai2b::COL_ENV_ROWS_MAX * B))) return rc;
	if ((rc = collision_counts_alloc(ctx))) return rc;
	const int env_rows = sai2b::col_env_rows(cfg->n_planes, cfg->n_obstacles);
	// the rows go into the buffer only now that nothing can be refused any more; a copy that fails leaves no configuration
	ctx->col_on = false;
	if (env_rows > 0) {
		if (rows) {
			if ((rc = copy_rows(ctx, ctx->col_env, rows, env_rows, on_device))) return rc;
		} else {
			const std::vector<double> absent((size_t)env_rows * B, std::nan(""));
			if ((rc = copy_rows(ctx, ctx->col_env, absent.data(), env_rows, 0))) return rc;
		}
	}
	HIP_TRY(ctx, hipMemsetAsync(ctx->col_counts, 0, sai2b::COL_COUNTS * sizeof(int), ctx->stream));
	sai2b::ColParams p;
	sai2b::ColLaw<N>& L = p.law;
	const sai2b::DevModel& m = ctx->h_params.model;
	for (int i = 0; i < N; i++) {
		for (int a = 0; a < 9; a++) L.E[i][a] = m.E[i][a];
		for (int a = 0; a < 3; a++) L.xyz[i][a] = m.xyz[i][a];
		L.jtype[i] = m.jtype[i];
	}
	L.n_spheres = cfg->n_spheres, L.n_planes = cfg->n_planes, L.n_obstacles = cfg->n_obstacles, L.blocks = cfg->blocks;
	L.env_mask = cfg->env_mask;
	for (int k = 0; k < SAI2B_MAX_COLLISION_SPHERES; k++) {
		const bool on = k < cfg->n_spheres;
		L.pair_mask[k] = on ? cfg->pair_mask[k] : 0u;
		L.link[k] = on ? cfg->link[k] : -1;
		for (int a = 0; a < 3; a++) L.centre[k][a] = on ? cfg->centre[k][a] : 0.0;
		L.radius[k] = on ? cfg->radius[k] : 0.0;
	}
	L.margin[0] = cfg->margin_plane, L.margin[1] = cfg->margin_obstacle, L.margin[2] = cfg->margin_self;
	ctx->col_rows = sai2b::col_layout(cfg->blocks, N, cfg->n_spheres, L.row);
	ctx->col_env_rows = env_rows;
	ctx->col = p;
	ctx->col_cfg = *cfg;
	std::memset(ctx->col_cfg.reserved, 0, sizeof(ctx->col_cfg.reserved));
	ctx->col_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_collision(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_collision: null ctx");
	if (ctx->body_on)  // the body is the collision's geometry: it goes with it
		if (int rc = sai2b_clear_body_contact(ctx)) return rc;
	ctx->col_on = false;
	ctx->col_rows = ctx->col_env_rows = 0;
	return SAI2B_OK;
}
extern "C" int sai2b_get_collision(sai2b_ctx* ctx, sai2b_collision_config* cfg, double* rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_collision: null ctx");
	if (!ctx->col_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_collision: no collision geometry is configured (sai2b_set_collision)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (cfg) *cfg = ctx->col_cfg;
	if (ctx->col_env_rows == 0) return SAI2B_OK;
	return fetch_rows(ctx, ctx->col_env, 0, ctx->col_env_rows, rows);
}
extern "C" int sai2b_collision_rows(sai2b_ctx* ctx) { return ctx && ctx->col_on ? ctx->col_rows : -1; }
extern "C" int sai2b_collision_layout(sai2b_ctx* ctx, int block, int category, int* first_row, int* n_rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_collision_layout: null ctx");
	if (!ctx->col_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_collision_layout: no collision geometry is configured (sai2b_set_collision)");
	const int rc = sai2b_collision_config_layout(&ctx->col_cfg, N, block, category, first_row, n_rows, nullptr, nullptr);
	return rc ? set_error(ctx, rc, g_error) : SAI2B_OK;
}
extern "C" int sai2b_collision_query(sai2b_ctx* ctx, double* out, unsigned char* flags, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_collision_query: null ctx");
	if (!ctx->col_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_collision_query: no collision geometry is configured (sai2b_set_collision)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc;
	const size_t B = ctx->B;
	const bool want_out = out && ctx->col_rows > 0;
	double* d_out = want_out ? out : nullptr;
	unsigned char* d_flags = flags;
	if (on_device) {
		// device results are written on the ctx stream: what the caller's stream still does with those buffers comes first
		if ((want_out || flags) && (rc = caller_before_read(ctx))) return rc;
	} else {
		if (want_out) {
			if (ctx->col_out_rows < ctx->col_rows) {  // a configuration with more rows: the smaller staging buffer goes
				if (ctx->col_out) {
					HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), (void*)ctx->col_out), ctx->allocs.end());
					HIP_TRY(ctx, hipFree(ctx->col_out));
					ctx->col_out = nullptr, ctx->col_out_rows = 0;
				}
				if ((rc = dev_alloc(ctx, &ctx->col_out, (size_t)ctx->col_rows * B))) return rc;
				ctx->col_out_rows = ctx->col_rows;
			}
			d_out = ctx->col_out;
		}
		if (flags) {
			if (!ctx->col_flags && (rc = dev_alloc(ctx, &ctx->col_flags, B))) return rc;
			d_flags = ctx->col_flags;
		}
	}
	HIP_TRY(ctx, hipMemsetAsync(ctx->col_counts, 0, sai2b::COL_COUNTS * sizeof(int), ctx->stream));
	sai2b::ColParams p = ctx->col;
	p.q = ctx->col_cfg.view == 1 ? ctrl_q(ctx) : ctx->q;
	p.rows = ctx->col_env_rows > 0 ? ctx->col_env : nullptr;
	p.out = d_out, p.flags = d_flags, p.counts = ctx->col_counts;
	if (sai2b::launch_collision(ctx->B, p, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "sai2b_collision_query: launch failed");
	ctx->launches++;
	if (on_device) return (want_out || flags) ? caller_after_read(ctx) : SAI2B_OK;
	if (want_out) HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)ctx->col_rows * B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (flags) HIP_TRY(ctx, hipMemcpyAsync(flags, d_flags, B, hipMemcpyDeviceToHost, ctx->stream));
	if (want_out || flags) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_collision_counts(sai2b_ctx* ctx, int counts[5]) {
	if (!ctx || !counts) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_collision_counts: bad arguments");
	if (!ctx->col_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_collision_counts: no collision geometry is configured (sai2b_set_collision)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->col_counts, sai2b::COL_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

// ---- whole-arm contact of the simulated plant (include/sai2b.h "whole-arm contact"; law: sai2b_body_contact_law.h; kernel:
// sai2b_sim.hip: sim_body_kernel) ----
static_assert(sai2b::COL_MAX_SPHERES == SAI2B_MAX_COLLISION_SPHERES, "sai2b_collision_law.h and sai2b.h disagree about the spheres");
extern "C" int sai2b_default_body_contact(sai2b_body_contact_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_body_contact: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	cfg->categories = (1 << SAI2B_COL_PLANE) | (1 << SAI2B_COL_OBSTACLE) | (1 << SAI2B_COL_SELF);
	cfg->v_eps = 1e-3;
	return SAI2B_OK;
}
static std::string body_contact_config_error(const sai2b_body_contact_config* c) {
	if (!c) return "body contact: null config";
	const int all = (1 << SAI2B_COL_PLANE) | (1 << SAI2B_COL_OBSTACLE) | (1 << SAI2B_COL_SELF);
	if (c->categories & ~all) return "body contact: unknown bits in categories";
	if (!(c->categories & all)) return "body contact: categories selects nothing";
	if (!std::isfinite(c->v_eps) || !(c->v_eps > 0)) return "body contact: v_eps must be finite and > 0";
	return "";
}
extern "C" int sai2b_validate_body_contact(const sai2b_body_contact_config* cfg, int robot_dof, char* msg, int msg_len) {
	const std::string err = robot_dof == N ? body_contact_config_error(cfg) : "body contact: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (err.empty()) return SAI2B_OK;
	return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_validate_body_contact: " + err);
}
extern "C" int sai2b_sizeof_body_contact_config(void) { return (int)sizeof(sai2b_body_contact_config); }
extern "C" int sai2b_set_body_contact(sai2b_ctx* ctx, const sai2b_body_contact_config* cfg, const double* rows, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_body_contact: null ctx");
	std::string err = body_contact_config_error(cfg);
	const size_t B = ctx->B;
	if (err.empty() && !ctx->col_on) err = "body contact: needs a collision configuration (sai2b_set_collision)";
	if (err.empty() && !rows) err = "body contact: rows are required";
	if (err.empty() && !on_device)
		for (size_t i = 0; i < (size_t)sai2b::BC_ROWS * B; i++)
			if (!std::isfinite(rows[i]) || rows[i] < 0) {
				err = "body contact: stiffness, damping and friction must be finite and >= 0";
				break;
			}
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_" + err);
	int rc;
	if ((rc = flush_update(ctx))) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t status_rows = (size_t)sai2b::bc_status_rows(N);
	// three buffers, each created once: a failed allocation leaves the others for the next call, and the context as it was
	if (!ctx->body_rows && (rc = dev_alloc(ctx, &ctx->body_rows, (size_t)sai2b::BC_ROWS * B))) return rc;
	if (!ctx->body_status) {
		if ((rc = dev_alloc(ctx, &ctx->body_status, status_rows * B))) return rc;
		HIP_TRY(ctx, hipMemsetAsync(ctx->body_status, 0, status_rows * B * sizeof(double), ctx->stream));
	}
	if (!ctx->body_counts) {
		if ((rc = dev_alloc(ctx, &ctx->body_counts, (size_t)sai2b::BC_COUNTS))) return rc;
		HIP_TRY(ctx, hipMemsetAsync(ctx->body_counts, 0, sai2b::BC_COUNTS * sizeof(int), ctx->stream));
	}
	// rows already in force are rewritten in place: taken out of force first, so that a copy that fails leaves the plant without
	// the feature, never with rows that are half the old ones and half the new
	ctx->body_on = false;
	if ((rc = copy_rows(ctx, ctx->body_rows, rows, sai2b::BC_ROWS, on_device))) return rc;
	ctx->body_cfg = *cfg;
	ctx->body_cfg.reserved0 = 0;
	std::memset(ctx->body_cfg.reserved, 0, sizeof(ctx->body_cfg.reserved));
	ctx->body_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_body_contact(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_body_contact: null ctx");
	if (int rc = flush_update(ctx)) return rc;
	// the status of the last step with the feature does not outlive it: sai2b_get_body_contact_state gives zeros from here on
	if (ctx->body_status && ctx->body_counts) {
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		HIP_TRY(ctx, hipMemsetAsync(ctx->body_status, 0, (size_t)sai2b::bc_status_rows(N) * ctx->B * sizeof(double), ctx->stream));
		HIP_TRY(ctx, hipMemsetAsync(ctx->body_counts, 0, sai2b::BC_COUNTS * sizeof(int), ctx->stream));
	}
	ctx->body_on = false;
	return SAI2B_OK;
}
extern "C" int sai2b_get_body_contact(sai2b_ctx* ctx, sai2b_body_contact_config* cfg, double* rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_body_contact: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (cfg) {
		if (ctx->body_on)
			*cfg = ctx->body_cfg;
		else
			std::memset(cfg, 0, sizeof(*cfg));
	}
	if (!ctx->body_on) {
		if (rows) std::fill(rows, rows + (size_t)sai2b::BC_ROWS * ctx->B, 0.0);
		return SAI2B_OK;
	}
	return fetch_rows(ctx, ctx->body_rows, 0, sai2b::BC_ROWS, rows);
}
extern "C" int sai2b_get_body_contact_state(sai2b_ctx* ctx, double* status, int counts[4]) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_get_body_contact_state: null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t status_rows = (size_t)sai2b::bc_status_rows(N);
	if (!ctx->body_status || !ctx->body_counts) {  // never had it
		if (status) std::fill(status, status + status_rows * ctx->B, 0.0);
		if (counts) std::fill(counts, counts + sai2b::BC_COUNTS, 0);
		return SAI2B_OK;
	}
	if (int rc = fetch_rows(ctx, ctx->body_status, 0, status_rows, status)) return rc;
	if (counts) {
		HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->body_counts, sai2b::BC_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	return SAI2B_OK;
}
// what sim_body_kernel takes: the collision configuration's geometry as it is now, the live environment rows
static sai2b::BodyParams body_params(const sai2b_ctx* ctx) {
	sai2b::BodyParams p;
	sai2b::BcGeom& G = p.geom;
	const sai2b::ColLaw<N>& L = ctx->col.law;
	G.n_spheres = L.n_spheres, G.n_planes = L.n_planes, G.n_obstacles = L.n_obstacles;
	G.categories = ctx->body_cfg.categories;
	G.env_mask = L.env_mask;
	for (int a = 0; a < sai2b::COL_MAX_SPHERES; a++) {
		G.partner[a] = L.pair_mask[a];
		for (int b = 0; b < a; b++) G.partner[a] |= ((L.pair_mask[b] >> a) & 1u) << b;
		G.link[a] = L.link[a];
		for (int k = 0; k < 3; k++) G.centre[a][k] = L.centre[a][k];
		G.radius[a] = L.radius[a];
	}
	G.v_eps = ctx->body_cfg.v_eps;
	p.env = ctx->col_env_rows > 0 ? ctx->col_env : nullptr;
	p.rows = ctx->body_rows, p.status = ctx->body_status, p.counts = ctx->body_counts;
	return p;
}

extern "C" int sai2b_end_episodes(sai2b_ctx* ctx, unsigned char* done_inout, const unsigned char* extra, int bit, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_end_episodes: null ctx");
	if (bit != 64 && bit != 128) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_end_episodes: bit must be 64 or 128");
	if (!done_inout || !extra) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_end_episodes: done_inout and extra are required");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc;
	const size_t B = ctx->B;
	if ((rc = collision_counts_alloc(ctx))) return rc;
	sai2b::EndParams p;
	p.done = done_inout, p.extra = extra, p.bit = bit;
	if (on_device) {
		if ((rc = caller_before_read(ctx))) return rc;
	} else {
		if (!ctx->end_done && (rc = dev_alloc(ctx, &ctx->end_done, B))) return rc;
		if (!ctx->end_extra && (rc = dev_alloc(ctx, &ctx->end_extra, B))) return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->end_done, done_inout, B, hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->end_extra, extra, B, hipMemcpyHostToDevice, ctx->stream));
		p.done = ctx->end_done, p.extra = ctx->end_extra;
	}
	if (ctx->rew_on) p.state = ctx->rew_state, p.episode = ctx->rew_episode;
	if (ctx->obs_on) p.steps = ctx->obs_steps;
	p.count = ctx->col_counts + sai2b::COL_COUNTS;
	HIP_TRY(ctx, hipMemsetAsync(p.count, 0, sizeof(int), ctx->stream));
	if (sai2b::launch_end_episodes(ctx->B, p, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "sai2b_end_episodes: launch failed");
	ctx->launches++;
	if (on_device) return caller_after_read(ctx);
	HIP_TRY(ctx, hipMemcpyAsync(done_inout, ctx->end_done, B, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_end_episode_count(sai2b_ctx* ctx, int* count) {
	if (!ctx || !count) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_end_episode_count: bad arguments");
	*count = 0;
	if (!ctx->col_counts) return SAI2B_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(count, ctx->col_counts + sai2b::COL_COUNTS, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

// ------------------------------------------------------------------------------------------------
// inverse kinematics (include/sai2b.h "inverse kinematics"; law: sai2b_ik_law.h; kernel: sai2b_ik.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int sai2b_default_ik(sai2b_ik_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_ik: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	cfg->axes = 63, cfg->max_iterations = 40, cfg->use_limits = 1;
	cfg->rot_length = 0.25, cfg->tol_pos = cfg->tol_rot = 1e-6;
	cfg->mu0 = 1e-2, cfg->mu_min = 1e-9, cfg->mu_max = 1e3, cfg->mu_down = 0.25, cfg->mu_up = 8.0;
	cfg->step_max = 0.5;
	return SAI2B_OK;
}
// lower / upper: the model's limits or both NULL (not known yet: what hangs on them is not checked)
static std::string ik_config_error(const sai2b_ik_config* c, const double* lower, const double* upper) {
	if (!c) return "ik: null config";
	if (c->task < 0 || c->task >= SAI2B_MAX_TASKS) return "ik: task must be a task index";
	if (c->axes & ~63) return "ik: unknown bits in axes";
	if (!(c->axes & 63)) return "ik: axes selects no component";
	if (!std::isfinite(c->rot_length) || !(c->rot_length > 0)) return "ik: rot_length must be finite and > 0";
	if (c->max_iterations < 1 || c->max_iterations > SAI2B_IK_MAX_ITERATIONS) return "ik: max_iterations must be in [1, SAI2B_IK_MAX_ITERATIONS]";
	if (c->restarts < 0 || c->restarts > SAI2B_IK_MAX_RESTARTS) return "ik: restarts must be in [0, SAI2B_IK_MAX_RESTARTS]";
	if (!std::isfinite(c->tol_pos) || !std::isfinite(c->tol_rot) || c->tol_pos < 0 || c->tol_rot < 0) return "ik: tol_pos and tol_rot must be finite and >= 0";
	if (!std::isfinite(c->mu_min) || !std::isfinite(c->mu0) || !std::isfinite(c->mu_max) || !(c->mu_min > 0) || !(c->mu_min <= c->mu0) || !(c->mu0 <= c->mu_max))
		return "ik: damping needs 0 < mu_min <= mu0 <= mu_max, all finite";
	if (!(c->mu_down > 0) || !(c->mu_down < 1)) return "ik: mu_down must be in (0, 1)";
	if (!std::isfinite(c->mu_up) || !(c->mu_up > 1)) return "ik: mu_up must be finite and > 1";
	if (!std::isfinite(c->step_max) || !(c->step_max > 0)) return "ik: step_max must be finite and > 0";
	if (c->use_limits != 0 && c->use_limits != 1) return "ik: use_limits must be 0 or 1";
	if (!std::isfinite(c->limit_margin) || c->limit_margin < 0) return "ik: limit_margin must be finite and >= 0";
	if (!std::isfinite(c->rest_weight) || c->rest_weight < 0) return "ik: rest_weight must be finite and >= 0";
	if (c->view != 0 && c->view != 1) return "ik: view must be 0 (the plant's q) or 1 (the measured q)";
	if (c->goal_source != SAI2B_IK_ROWS && c->goal_source != SAI2B_IK_TASK_GOAL) return "ik: goal_source must be SAI2B_IK_ROWS or SAI2B_IK_TASK_GOAL";
	if (c->seed_source != SAI2B_IK_ROWS && c->seed_source != SAI2B_IK_STATE) return "ik: seed_source must be SAI2B_IK_ROWS or SAI2B_IK_STATE";
	if (c->restarts > 0 && !c->use_limits) return "ik: restarts need use_limits (the seeds are drawn inside the limits)";
	if (lower && upper && c->use_limits) {
		for (int i = 0; i < N; i++) {
			const double lo = lower[i] + c->limit_margin, hi = upper[i] - c->limit_margin;
			if (!(lo <= hi)) return "ik: limit_margin leaves a joint no interval (or a limit is NaN)";
			if (c->restarts > 0 && (!std::isfinite(lo) || !std::isfinite(hi))) return "ik: restarts need finite limits on every joint";
		}
	}
	return "";
}
extern "C" int sai2b_validate_ik(const sai2b_ik_config* cfg, int robot_dof, const double* q_lower, const double* q_upper, char* msg, int msg_len) {
	std::string err = robot_dof == N ? ik_config_error(cfg, q_lower, q_upper) : "ik: this build serves another robot size";
	if (err.empty() && (q_lower == nullptr) != (q_upper == nullptr)) err = "ik: q_lower and q_upper are given together or not at all";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (err.empty()) return SAI2B_OK;
	return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_validate_ik: " + err);
}
extern "C" int sai2b_sizeof_ik_config(void) { return (int)sizeof(sai2b_ik_config); }
extern "C" int sai2b_ik_input_rows(const sai2b_ik_config* cfg, int robot_dof, int* goal_rows, int* seed_rows) {
	if (robot_dof != N) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_ik_input_rows: this build serves another robot size");
	const std::string err = ik_config_error(cfg, nullptr, nullptr);
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_ik_input_rows: " + err);
	if (goal_rows) *goal_rows = (cfg->goal_source == SAI2B_IK_ROWS ? sai2b::IK_POSE_ROWS : 0) + (cfg->rest_weight > 0 ? N : 0);
	if (seed_rows) *seed_rows = cfg->seed_source == SAI2B_IK_ROWS ? N : 0;
	return SAI2B_OK;
}
static std::string ik_context_error(const sai2b_ctx* ctx, const sai2b_ik_config* cfg) {
	std::string err = ik_config_error(cfg, ctx->h_params.model.q_lower, ctx->h_params.model.q_upper);
	if (err.empty() && cfg->task >= ctx->T) err = "ik: task must be a task index";
	if (err.empty() && ctx->h_params.task[cfg->task].type != SAI2B_MOTION_FORCE_TASK) err = "ik: task must be a MotionForceTask";
	return err;
}
extern "C" int sai2b_set_ik(sai2b_ctx* ctx, const sai2b_ik_config* cfg) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_ik: null ctx");
	const std::string err = cfg ? ik_context_error(ctx, cfg) : "ik: null config";
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_" + err);
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!ctx->ik_counts) {
		if (int rc = dev_alloc(ctx, &ctx->ik_counts, (size_t)sai2b::IK_COUNTS)) return rc;
	}
	HIP_TRY(ctx, hipMemsetAsync(ctx->ik_counts, 0, sai2b::IK_COUNTS * sizeof(int), ctx->stream));
	ctx->ik_cfg = *cfg;
	std::memset(ctx->ik_cfg.reserved, 0, sizeof(ctx->ik_cfg.reserved));
	ctx->ik_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_ik(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_ik: null ctx");
	ctx->ik_on = false;
	return SAI2B_OK;
}
extern "C" int sai2b_get_ik(sai2b_ctx* ctx, sai2b_ik_config* cfg) {
	if (!ctx || !cfg) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_ik: bad arguments");
	if (!ctx->ik_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_ik: no inverse kinematics is configured (sai2b_set_ik)");
	*cfg = ctx->ik_cfg;
	return SAI2B_OK;
}
// the law's block from the configuration and the context's model and task as they stand
static void ik_fill_law(const sai2b_ctx* ctx, sai2b::IkLaw<N>& L) {
	const sai2b_ik_config& c = ctx->ik_cfg;
	const sai2b::DevModel& m = ctx->h_params.model;
	const DevTask& t = ctx->h_params.task[c.task];
	for (int i = 0; i < N; i++) {
		for (int a = 0; a < 9; a++) L.E[i][a] = m.E[i][a];
		for (int a = 0; a < 3; a++) L.xyz[i][a] = m.xyz[i][a];
		L.jtype[i] = m.jtype[i];
		L.lo[i] = c.use_limits ? m.q_lower[i] + c.limit_margin : -HUGE_VAL;
		L.hi[i] = c.use_limits ? m.q_upper[i] - c.limit_margin : HUGE_VAL;
	}
	L.link = t.link;
	for (int a = 0; a < 3; a++) L.frame_pos[a] = t.frame_pos[a];
	for (int a = 0; a < 9; a++) L.frame_rot[a] = t.frame_rot[a];
	for (int a = 0; a < 6; a++) {
		const bool on = (c.axes >> a) & 1;
		L.sel[a] = on ? 1.0 : 0.0;
		L.w2[a] = on ? (a < 3 ? 1.0 : c.rot_length * c.rot_length) : 0.0;
	}
	L.max_iterations = c.max_iterations, L.restarts = c.restarts, L.use_limits = c.use_limits;
	L.tol_pos = c.tol_pos, L.tol_rot = c.tol_rot;
	L.mu0 = c.mu0, L.mu_min = c.mu_min, L.mu_max = c.mu_max, L.mu_down = c.mu_down, L.mu_up = c.mu_up;
	L.step_max = c.step_max, L.rest_weight = c.rest_weight;
	L.key0 = (unsigned)(c.seed & 0xffffffffull), L.key1 = (unsigned)(c.seed >> 32);
	L.first_robot = c.first_robot, L.draw_id = c.draw_id;
}
extern "C" int sai2b_solve_ik(sai2b_ctx* ctx, const double* goal_rows, const double* seed_rows, const unsigned char* mask, double* q_out, double* status,
							  unsigned char* flags, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_solve_ik: null ctx");
	if (!ctx->ik_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_solve_ik: no inverse kinematics is configured (sai2b_set_ik)");
	const sai2b_ik_config& c = ctx->ik_cfg;
	// the model's limits or the task may have changed since sai2b_set_ik
	const std::string err = ik_context_error(ctx, &c);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_solve_" + err);
	const int pose_rows = c.goal_source == SAI2B_IK_ROWS ? sai2b::IK_POSE_ROWS : 0, rest_rows = c.rest_weight > 0 ? N : 0;
	const int g_rows = pose_rows + rest_rows, s_rows = c.seed_source == SAI2B_IK_ROWS ? N : 0;
	if (g_rows > 0 && !goal_rows) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_solve_ik: goal_rows is NULL");
	if (s_rows > 0 && !seed_rows) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_solve_ik: seed_rows is NULL");
	if (!q_out || !status || !flags) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_solve_ik: q_out, status and flags are required");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc;
	const size_t B = ctx->B;
	const double *d_goal = goal_rows, *d_seed = seed_rows;
	const unsigned char* d_mask = mask;
	double *d_q = q_out, *d_status = status;
	unsigned char* d_flags = flags;
	if (on_device) {
		if ((rc = caller_before_read(ctx))) return rc;
	} else {
		// staging, created on the first host call: goal 12 + N, seed N, q_out N, status 5 rows; mask and flags B bytes each
		constexpr size_t ROWS = sai2b::IK_POSE_ROWS + 3 * N + sai2b::IK_STATUS_ROWS;
		if (!ctx->ik_rows && (rc = dev_alloc(ctx, &ctx->ik_rows, ROWS * B))) return rc;
		if (!ctx->ik_bytes && (rc = dev_alloc(ctx, &ctx->ik_bytes, 2 * B))) return rc;
		double* r = ctx->ik_rows;
		if (g_rows > 0) HIP_TRY(ctx, hipMemcpyAsync(r, goal_rows, (size_t)g_rows * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		d_goal = r, r += (size_t)(sai2b::IK_POSE_ROWS + N) * B;
		if (s_rows > 0) HIP_TRY(ctx, hipMemcpyAsync(r, seed_rows, (size_t)N * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		d_seed = r, r += (size_t)N * B;
		HIP_TRY(ctx, hipMemcpyAsync(r, q_out, (size_t)N * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		d_q = r, r += (size_t)N * B;
		HIP_TRY(ctx, hipMemcpyAsync(r, status, (size_t)sai2b::IK_STATUS_ROWS * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		d_status = r;
		if (mask) {
			HIP_TRY(ctx, hipMemcpyAsync(ctx->ik_bytes, mask, B, hipMemcpyHostToDevice, ctx->stream));
			d_mask = ctx->ik_bytes;
		}
		d_flags = ctx->ik_bytes + B;
		HIP_TRY(ctx, hipMemcpyAsync(d_flags, flags, B, hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // pageable host memory may be reused by the caller
	}
	HIP_TRY(ctx, hipMemsetAsync(ctx->ik_counts, 0, sai2b::IK_COUNTS * sizeof(int), ctx->stream));
	sai2b::IkParams p;
	ik_fill_law(ctx, p.law);
	p.goal = pose_rows ? d_goal : ctx->h_params.task[c.task].goals;
	p.rest = rest_rows ? d_goal + (size_t)pose_rows * B : nullptr;
	p.seed = s_rows ? d_seed : (c.view == 1 ? ctrl_q(ctx) : ctx->q);
	p.mask = d_mask, p.q_out = d_q, p.status = d_status, p.flags = d_flags, p.counts = ctx->ik_counts;
	if (sai2b::launch_ik(ctx->B, p, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "sai2b_solve_ik: launch failed");
	ctx->launches++;
	if (on_device) return caller_after_read(ctx);
	HIP_TRY(ctx, hipMemcpyAsync(q_out, d_q, (size_t)N * B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(status, d_status, (size_t)sai2b::IK_STATUS_ROWS * B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(flags, d_flags, B, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}
extern "C" int sai2b_get_ik_counts(sai2b_ctx* ctx, int counts[4]) {
	if (!ctx || !counts) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_ik_counts: bad arguments");
	if (!ctx->ik_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_ik_counts: no inverse kinematics is configured (sai2b_set_ik)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->ik_counts, sai2b::IK_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

// ---- actions ----
namespace {
constexpr int ACT_ALL_BLOCKS = SAI2B_ACT_POSITION | SAI2B_ACT_ORIENTATION | SAI2B_ACT_FORCE | SAI2B_ACT_MOMENT;
int action_task_rows(const sai2b_action_task& a, const sai2b_task_config& t) {
	if (a.mode == SAI2B_ACT_NONE) return 0;
	if (t.type == SAI2B_JOINT_TASK) return t.task_dof;
	int rows = 0;
	for (int k = 0; k < sai2b::ACT_BLOCKS; k++)
		if ((a.blocks >> k) & 1) rows += 3;
	return rows;
}
// first action row of every task (-1: the task takes none); returns the rows of the whole action
int action_rows(const sai2b_action_config& c, const sai2b_task_config* tasks, int n_tasks, int row_task[SAI2B_MAX_TASKS]) {
	int rows = 0;
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) {
		const int n = t < n_tasks ? action_task_rows(c.task[t], tasks[t]) : 0;
		row_task[t] = n ? rows : -1;
		rows += n;
	}
	return rows;
}
bool bad_scale(double v) { return !std::isfinite(v) || v < 0; }
std::string action_config_error(const sai2b_action_config* c, const sai2b_task_config* tasks, int n_tasks) {
	if (!c) return "action: null config";
	if (!tasks || n_tasks < 1 || n_tasks > SAI2B_MAX_TASKS) return "action: no tasks to validate against";
	bool any = false;
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) {
		const sai2b_action_task& a = c->task[t];
		const std::string who = "action: task " + std::to_string(t) + ": ";
		if (a.mode < SAI2B_ACT_NONE || a.mode > SAI2B_ACT_ABSOLUTE) return who + "unknown mode";
		if (a.blocks & ~ACT_ALL_BLOCKS) return who + "unknown bits in blocks";
		if (a.mode == SAI2B_ACT_NONE) continue;
		if (t >= n_tasks) return who + "a mode on a task the hierarchy does not have";
		any = true;
		if (tasks[t].type == SAI2B_JOINT_TASK) {
			if (a.blocks) return who + "blocks are for a MotionForceTask (a JointTask takes task_dof rows)";
			for (int i = 0; i < tasks[t].task_dof && i < SAI2B_MAX_DOF; i++) {
				if (bad_scale(a.jt_scale[i])) return who + "jt_scale must be finite and >= 0";
				if (!(a.jt_lower[i] < a.jt_upper[i])) return who + "jt_lower must be < jt_upper (and neither a NaN)";
			}
			continue;
		}
		if (tasks[t].type != SAI2B_MOTION_FORCE_TASK) return who + "not a JointTask or MotionForceTask";
		if (!a.blocks) return who + "a MotionForceTask with a mode needs a block";
		if (bad_scale(a.pos_scale[0]) || bad_scale(a.pos_scale[1]) || bad_scale(a.pos_scale[2])) return who + "pos_scale must be finite and >= 0";
		if (bad_scale(a.ori_scale)) return who + "ori_scale must be finite and >= 0";
		if (bad_scale(a.force_scale)) return who + "force_scale must be finite and >= 0";
		if (bad_scale(a.moment_scale)) return who + "moment_scale must be finite and >= 0";
		for (int k = 0; k < 3; k++)
			if (!(a.pos_lower[k] < a.pos_upper[k])) return who + "pos_lower must be < pos_upper (and neither a NaN)";
		if (!(a.max_pos_lead > 0)) return who + "max_pos_lead must be > 0";
	}
	if (!any) return "action: no task has a mode";
	return "";
}
}  // namespace
extern "C" int sai2b_default_action(sai2b_action_config* cfg) {
	if (!cfg) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_default_action: null config");
	std::memset(cfg, 0, sizeof(*cfg));
	for (sai2b_action_task& a : cfg->task) {
		a.ori_scale = a.force_scale = a.moment_scale = 1.0;
		a.max_pos_lead = INFINITY;
		for (int k = 0; k < 3; k++) a.pos_scale[k] = 1.0, a.pos_lower[k] = -INFINITY, a.pos_upper[k] = INFINITY;
		for (int i = 0; i < SAI2B_MAX_DOF; i++) a.jt_scale[i] = 1.0, a.jt_lower[i] = -INFINITY, a.jt_upper[i] = INFINITY;
	}
	return SAI2B_OK;
}
extern "C" int sai2b_sizeof_action_config(void) { return (int)sizeof(sai2b_action_config); }
extern "C" int sai2b_validate_action(const sai2b_action_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof, char* msg,
									 int msg_len) {
	const std::string err = robot_dof == N ? action_config_error(cfg, tasks, n_tasks) : "action: this build serves another robot size";
	if (msg && msg_len > 0) std::snprintf(msg, msg_len, "%s", err.c_str());
	if (!err.empty()) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, err);
	return SAI2B_OK;
}
extern "C" int sai2b_action_config_layout(const sai2b_action_config* cfg, const sai2b_task_config* tasks, int n_tasks, int block, int task,
										  int* first_row, int* n_rows, int* total_rows) {
	if (!cfg || !tasks || n_tasks < 1 || n_tasks > SAI2B_MAX_TASKS)
		return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_action_config_layout: bad arguments");
	if (task < 0 || task >= n_tasks) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_action_config_layout: task must be a task index");
	const bool joint = tasks[task].type == SAI2B_JOINT_TASK;
	const int k = joint ? 0 : single_bit_index(block, sai2b::ACT_BLOCKS);
	if (k < 0) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_action_config_layout: block must be one known flag");
	int row_task[SAI2B_MAX_TASKS];
	const int rows = action_rows(*cfg, tasks, n_tasks, row_task);
	const sai2b_action_task& a = cfg->task[task];
	int first = -1, n = 0;
	if (row_task[task] >= 0) {
		if (joint) {
			first = row_task[task], n = tasks[task].task_dof;
		} else if ((a.blocks >> k) & 1) {
			first = row_task[task], n = 3;
			for (int j = 0; j < k; j++)
				if ((a.blocks >> j) & 1) first += 3;
		}
	}
	if (first_row) *first_row = first;
	if (n_rows) *n_rows = n;
	if (total_rows) *total_rows = rows;
	return SAI2B_OK;
}
extern "C" int sai2b_set_action(sai2b_ctx* ctx, const sai2b_action_config* cfg) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_set_action: null ctx");
	const std::string err = action_config_error(cfg, ctx->cfg, ctx->T);
	if (!err.empty()) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_" + err);
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc;
	if (!ctx->act_counts && (rc = dev_alloc(ctx, &ctx->act_counts, (size_t)sai2b::ACT_COUNTS))) return rc;
	HIP_TRY(ctx, hipMemsetAsync(ctx->act_counts, 0, sai2b::ACT_COUNTS * sizeof(int), ctx->stream));
	sai2b::ActParams p;
	int row_task[SAI2B_MAX_TASKS];
	p.rows = ctx->act_rows = action_rows(*cfg, ctx->cfg, ctx->T, row_task);
	p.clip = cfg->clip_actions != 0;
	for (int t = 0; t < ctx->T; t++) {
		const sai2b_action_task& a = cfg->task[t];
		sai2b::ActTask& d = p.task[t];
		if (a.mode == SAI2B_ACT_NONE) continue;
		const bool joint = ctx->cfg[t].type == SAI2B_JOINT_TASK;
		d.mode = a.mode, d.blocks = joint ? 0 : a.blocks, d.row = row_task[t];
		for (int k = 0; k < 3; k++) d.pos_scale[k] = a.pos_scale[k], d.pos_lower[k] = a.pos_lower[k], d.pos_upper[k] = a.pos_upper[k];
		d.ori_scale = a.ori_scale, d.force_scale = a.force_scale, d.moment_scale = a.moment_scale, d.max_lead = a.max_pos_lead;
		for (int i = 0; i < N; i++) d.jt_scale[i] = a.jt_scale[i], d.jt_lower[i] = a.jt_lower[i], d.jt_upper[i] = a.jt_upper[i];
		const bool lead = !joint && (a.blocks & SAI2B_ACT_POSITION) && a.max_pos_lead < INFINITY;
		if (a.mode == SAI2B_ACT_DELTA_CURRENT || lead) p.need_state = 1;
		if (!joint && (a.mode == SAI2B_ACT_DELTA_CURRENT || lead)) p.need_pose = 1;
	}
	ctx->act = p;
	ctx->act_cfg = *cfg;
	ctx->act_on = true;
	return SAI2B_OK;
}
extern "C" int sai2b_clear_action(sai2b_ctx* ctx) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_clear_action: null ctx");
	ctx->act_on = false;
	ctx->act_rows = 0;
	return SAI2B_OK;
}
extern "C" int sai2b_action_rows(sai2b_ctx* ctx) { return ctx && ctx->act_on ? ctx->act_rows : -1; }
extern "C" int sai2b_action_layout(sai2b_ctx* ctx, int block, int task, int* first_row, int* n_rows) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_action_layout: null ctx");
	if (!ctx->act_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_action_layout: no action is configured (sai2b_set_action)");
	const int rc = sai2b_action_config_layout(&ctx->act_cfg, ctx->cfg, ctx->T, block, task, first_row, n_rows, nullptr);
	return rc ? set_error(ctx, rc, g_error) : SAI2B_OK;
}
extern "C" int sai2b_apply_action(sai2b_ctx* ctx, const double* action, const unsigned char* mask, int on_device) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_apply_action: null ctx");
	if (!ctx->act_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_apply_action: no action is configured (sai2b_set_action)");
	if (!action) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_apply_action: action is NULL");
	int rc = flush_update(ctx);	 // DELTA_CURRENT reads the state: a deferred model update happens first
	if (rc) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if ((rc = upload_params(ctx))) return rc;
	const size_t B = ctx->B;
	const double* d_action = action;
	const unsigned char* d_mask = mask;
	if (on_device) {
		if ((rc = caller_before_read(ctx))) return rc;
	} else {
		if (ctx->act_in_rows < ctx->act_rows) {	 // a configuration with more rows: the smaller staging buffer goes
			if (ctx->act_in) {
				HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
				ctx->allocs.erase(std::remove(ctx->allocs.begin(), ctx->allocs.end(), (void*)ctx->act_in), ctx->allocs.end());
				HIP_TRY(ctx, hipFree(ctx->act_in));
				ctx->act_in = nullptr, ctx->act_in_rows = 0;
			}
			if ((rc = dev_alloc(ctx, &ctx->act_in, (size_t)ctx->act_rows * B))) return rc;
			ctx->act_in_rows = ctx->act_rows;
		}
		HIP_TRY(ctx, hipMemcpyAsync(ctx->act_in, action, (size_t)ctx->act_rows * B * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		d_action = ctx->act_in;
		if (mask) {
			if (!ctx->act_mask && (rc = dev_alloc(ctx, &ctx->act_mask, B))) return rc;
			HIP_TRY(ctx, hipMemcpyAsync(ctx->act_mask, mask, B, hipMemcpyHostToDevice, ctx->stream));
			d_mask = ctx->act_mask;
		}
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // pageable host memory may be reused by the caller
	}
	HIP_TRY(ctx, hipMemsetAsync(ctx->act_counts, 0, sai2b::ACT_COUNTS * sizeof(int), ctx->stream));
	if (sai2b::launch_action(ctrl_params(ctx), ctx->B, ctx->act, d_action, d_mask, ctx->act_counts, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "sai2b_apply_action: launch failed");
	// as the goal setters: the generators of the tasks that took rows compare their goals at the next tick
	for (int t = 0; t < ctx->T; t++)
		if (ctx->act_cfg.task[t].mode != SAI2B_ACT_NONE) ctx->goals_dirty |= 1u << t;
	ctx->goals_epoch++, ctx->otg_all_idle = false;
	ctx->launches++;
	return on_device ? caller_after_read(ctx) : SAI2B_OK;
}
extern "C" int sai2b_get_action_counts(sai2b_ctx* ctx, int counts[3]) {
	if (!ctx || !counts) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_action_counts: bad arguments");
	if (!ctx->act_on) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_action_counts: no action is configured (sai2b_set_action)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->act_counts, sai2b::ACT_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

// ---- simulation harness ----
extern "C" int sai2b_sim_step(sai2b_ctx* ctx, const double* tau, int on_device, double dt, int substeps, int with_gravity) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;
	if (!(dt > 0) || substeps < 1 || substeps > 1000) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_sim_step: dt must be > 0 and substeps in [1, 1000]");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = upload_params(ctx);
	if (rc) return rc;
	const double* t = ctx->tau;	 // default: the torques of the last computeControlTorques
	const bool caller_tau = tau && on_device;
	if (caller_tau) {
		t = tau;
		if ((rc = caller_before_read(ctx))) return rc;
	} else if (tau) {
		if (!ctx->sim_tau && (rc = dev_alloc(ctx, &ctx->sim_tau, (size_t)N * ctx->B))) return rc;
		if ((rc = copy_rows(ctx, ctx->sim_tau, tau, N, 0))) return rc;
		t = ctx->sim_tau;
	}
	// the kernel saves the pose the tasks cached (q_pose) on its way in, when the state buffer still holds it; with a joint sensor
	// the cached pose is the measured q, which the sense stage saves before it overwrites the measurement
	double* q_keep = ctx->q_is_pose ? ctx->q_pose : nullptr;
	ctx->q_is_pose = false;
	double* js_keep = nullptr;
	if (ctx->js_on) js_keep = q_keep, q_keep = nullptr;
	// the instantiation for what the context has set: plant payload, contact (whose counter starts each step at zero)
	const DevParams& hp = ctx->h_params;
	if (hp.contact) HIP_TRY(ctx, hipMemsetAsync(hp.contact_count, 0, sizeof(int), ctx->stream));
	// joint dynamics: sim_joint_kernel, its two counters zeroed alike
	if (ctx->joint_on) HIP_TRY(ctx, hipMemsetAsync(ctx->joint_counts, 0, sai2b::JOINT_COUNTS * sizeof(int), ctx->stream));
	// external wrench: the wrench forms of either kernel, the counter of robots pushed zeroed alike
	if (ctx->wrench_on) HIP_TRY(ctx, hipMemsetAsync(ctx->wrench_count, 0, sizeof(int), ctx->stream));
	// whole-arm contact: sim_body_kernel for every form, its four counters zeroed alike
	const bool body_on = ctx->body_on && ctx->col_on;
	sai2b::BodyParams body;
	if (body_on) {
		body = body_params(ctx);
		HIP_TRY(ctx, hipMemsetAsync(ctx->body_counts, 0, sai2b::BC_COUNTS * sizeof(int), ctx->stream));
	}
	// hardware: actuate_kernel turns the command into the applied torques, which the simulation kernel receives as its tau
	if (ctx->hw_on) {
		sai2b::ActuateParams a;
		a.rows = ctx->hw_act, a.command = t, a.history = ctx->hw_history, a.filter = ctx->hw_filter, a.applied = ctx->hw_applied;
		a.clock = ctx->hw_clock, a.depth = ctx->hw_cfg.max_delay, a.rng = hardware_stream(ctx);
		if (sai2b::launch_actuate(ctx->B, a, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "actuation launch failed");
		ctx->launches++;
		t = ctx->hw_applied;
	}
	if (sai2b::launch_sim(ctx->d_params, ctx->B, t, dt, substeps, with_gravity, hp.plant_payload != nullptr, hp.contact != nullptr,
						  ctx->joint_on ? &ctx->joint : nullptr, ctx->wrench_on ? &ctx->wrench : nullptr, body_on ? &body : nullptr, nullptr, q_keep,
						  ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "simulation launch failed");
	ctx->launches++;
	// hardware: sense_kernel, only when the simulation kernel has just written the ideal reading into the sensor's task
	const int hw_task = ctx->hw_on ? ctx->hw_cfg.sensor_task : -1;
	if (hw_task >= 0 && ((hp.contact && hp.contact_sensor_task == hw_task) || (ctx->wrench_on && ctx->wrench_cfg.sensor_task == hw_task))) {
		sai2b::SenseParams s;
		s.rows = ctx->hw_sensor, s.sensed = hp.task[hw_task].sensed, s.filter = ctx->hw_filter, s.clock = ctx->hw_clock, s.rng = hardware_stream(ctx);
		if (sai2b::launch_sense(ctx->B, s, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "sensor launch failed");
		ctx->launches++;
	}
	// joint sensors: the next reading of the state the plant has just reached, last in the call
	if (ctx->js_on) {
		sai2b::JointSenseParams s = joint_sense_params(ctx);
		s.dt = dt, s.q_pose = js_keep;
		if (sai2b::launch_joint_sense(ctx->B, s, false, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, "joint sensor launch failed");
		ctx->launches++;
	}
	ctx->models_fresh = false;
	for (int k = 0; k < ctx->T; k++) ctx->tio[k].model_fresh = false;
	if (caller_tau) return caller_after_read(ctx);
	return SAI2B_OK;
}
extern "C" int sai2b_get_state(sai2b_ctx* ctx, double* q, double* dq) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = fetch_rows(ctx, ctx->q, 0, N, q);
	if (rc) return rc;
	return fetch_rows(ctx, ctx->dq, 0, N, dq);
}
extern "C" int sai2b_get_bias(sai2b_ctx* ctx, int with_gravity, double* bias) {
	if (!ctx || !bias) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_bias: bad arguments");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = upload_params(ctx);
	if (rc) return rc;
	if (!ctx->sim_tau && (rc = dev_alloc(ctx, &ctx->sim_tau, (size_t)N * ctx->B))) return rc;
	// a zero-length step leaves the state as it is and writes the bias vector of the current state
	if (sai2b::launch_sim(ctx->d_params, ctx->B, nullptr, 0.0, 1, with_gravity, ctx->h_params.plant_payload != nullptr, false, nullptr, nullptr, nullptr, ctx->sim_tau, nullptr, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "simulation launch failed");
	return fetch_rows(ctx, ctx->sim_tau, 0, N, bias);
}

static int run_status(sai2b_ctx* ctx, int task) {
	int rc = flush_update(ctx);	 // a deferred model update (and its launch errors) happens before anything is observed
	if (rc) return rc;
	rc = upload_params(ctx);
	if (rc) return rc;
	if (!ctx->status_buf && (rc = dev_alloc(ctx, &ctx->status_buf, 68 * (size_t)ctx->B))) return rc;
	if (sai2b::launch_mft_status(ctrl_params(ctx), ctx->B, task, ctx->status_buf, ctx->stream))
		return set_error(ctx, SAI2B_RUNTIME_ERROR, "status launch failed");
	return SAI2B_OK;
}
extern "C" int sai2b_get_mft_velocity(sai2b_ctx* ctx, int task, double* linear_velocity, double* angular_velocity) {
	int rc = mft_task_check(ctx, task, "sai2b_get_mft_velocity");
	if (rc) return rc;
	if ((rc = run_status(ctx, task))) return rc;
	if ((rc = fetch_rows(ctx, ctx->status_buf, 26, 3, linear_velocity))) return rc;
	return fetch_rows(ctx, ctx->status_buf, 29, 3, angular_velocity);
}
extern "C" int sai2b_get_mft_sigma(sai2b_ctx* ctx, int task, double* sigma_force, double* sigma_position, double* sigma_moment,
								   double* sigma_orientation) {
	int rc = mft_task_check(ctx, task, "sai2b_get_mft_sigma");
	if (rc) return rc;
	if ((rc = run_status(ctx, task))) return rc;
	if ((rc = fetch_rows(ctx, ctx->status_buf, 32, 9, sigma_force))) return rc;
	if ((rc = fetch_rows(ctx, ctx->status_buf, 41, 9, sigma_position))) return rc;
	if ((rc = fetch_rows(ctx, ctx->status_buf, 50, 9, sigma_moment))) return rc;
	return fetch_rows(ctx, ctx->status_buf, 59, 9, sigma_orientation);
}
// SingularityHandler::setType1Posture (SingularityHandler.h:140-142, via MotionForceTask.h:706): _q_prior := q_des.
// Like the reference's member it holds until the handler next refreshes it (on entering a singular region, or
// while type-2 classifications dominate: SingularityHandler.cpp:233-236).
extern "C" int sai2b_set_mft_type1_posture(sai2b_ctx* ctx, int task, const double* q_des, int on_device) {
	int rc = mft_task_check(ctx, task, "sai2b_set_mft_type1_posture");
	if (rc) return rc;
	if ((rc = flush_update(ctx))) return rc;
	if (!q_des) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_set_mft_type1_posture: null posture");
	return copy_rows(ctx, ctx->h_params.task[task].state + (size_t)sai2b::MFT_QPRIOR * ctx->B, q_des, N, on_device);
}
extern "C" int sai2b_get_mft_status(sai2b_ctx* ctx, int task, double* pos, double* rot, double* sensed_force_world,
									double* sensed_moment_world, double* pos_error, double* ori_error, double* pos_error_norm,
									double* ori_error_norm) {
	int rc = mft_task_check(ctx, task, "sai2b_get_mft_status");
	if (rc) return rc;
	if ((rc = run_status(ctx, task))) return rc;
	const double* S = ctx->status_buf;
	if ((rc = fetch_rows(ctx, S, 0, 3, pos))) return rc;
	if ((rc = fetch_rows(ctx, S, 3, 9, rot))) return rc;
	if ((rc = fetch_rows(ctx, S, 12, 3, sensed_force_world))) return rc;
	if ((rc = fetch_rows(ctx, S, 15, 3, sensed_moment_world))) return rc;
	if ((rc = fetch_rows(ctx, S, 18, 3, pos_error))) return rc;
	if ((rc = fetch_rows(ctx, S, 21, 3, ori_error))) return rc;
	if ((rc = fetch_rows(ctx, S, 24, 1, pos_error_norm))) return rc;
	return fetch_rows(ctx, S, 25, 1, ori_error_norm);
}
extern "C" int sai2b_get_mft_goals(sai2b_ctx* ctx, int task, double* pos, double* rot, double* lin_vel, double* ang_vel,
								   double* lin_acc, double* ang_acc, double* force, double* moment) {
	int rc = mft_task_check(ctx, task, "sai2b_get_mft_goals");
	if (rc) return rc;
	const double* G = ctx->h_params.task[task].goals;
	double* dst[8] = {pos, rot, lin_vel, ang_vel, lin_acc, ang_acc, force, moment};
	using namespace sai2b;
	const size_t row0[8] = {MFT_GOAL_POS, MFT_GOAL_ROT, MFT_GOAL_LIN_VEL, MFT_GOAL_ANG_VEL, MFT_GOAL_LIN_ACC, MFT_GOAL_ANG_ACC, MFT_GOAL_FORCE, MFT_GOAL_MOMENT};
	const size_t rows[8] = {3, 9, 3, 3, 3, 3, 3, 3};
	for (int k = 0; k < 8; k++)
		if ((rc = fetch_rows(ctx, G, row0[k], rows[k], dst[k]))) return rc;
	return SAI2B_OK;
}
extern "C" int sai2b_get_jt_goals(sai2b_ctx* ctx, int task, double* q, double* dq, double* ddq) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (task < 0 || task >= ctx->T || ctx->cfg[task].type != SAI2B_JOINT_TASK)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_jt_goals: task is not a JointTask");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const double* G = ctx->h_params.task[task].goals;
	const size_t k0 = ctx->cfg[task].task_dof;
	int rc;
	if ((rc = fetch_rows(ctx, G, 0, k0, q))) return rc;
	if ((rc = fetch_rows(ctx, G, k0, k0, dq))) return rc;
	return fetch_rows(ctx, G, 2 * k0, k0, ddq);
}

extern "C" int sai2b_reset_integrators(sai2b_ctx* ctx, int task, int which) {
	if (!ctx || task < 0 || task >= ctx->T) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_reset_integrators: bad arguments");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	double* S = ctx->h_params.task[task].state;
	const size_t B = ctx->B, row = B * sizeof(double);
	if (ctx->cfg[task].type == SAI2B_JOINT_TASK) {
		HIP_TRY(ctx, hipMemsetAsync(S, 0, row * ctx->cfg[task].task_dof, ctx->stream));
		return SAI2B_OK;
	}
	// MFT state rows: integral of position 0-2, orientation 3-5, force 6-8, moment 9-11
	if (which == 0 || which == 1) {
		HIP_TRY(ctx, hipMemsetAsync(S, 0, row * 3, ctx->stream));
		HIP_TRY(ctx, hipMemsetAsync(S + 6 * B, 0, row * 3, ctx->stream));
	}
	if (which == 0 || which == 2) {
		HIP_TRY(ctx, hipMemsetAsync(S + 3 * B, 0, row * 3, ctx->stream));
		HIP_TRY(ctx, hipMemsetAsync(S + 9 * B, 0, row * 3, ctx->stream));
	}
	return SAI2B_OK;
}

extern "C" int sai2b_get_jt_desired(sai2b_ctx* ctx, int task, double* q, double* dq, double* ddq) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (task < 0 || task >= ctx->T || ctx->cfg[task].type != SAI2B_JOINT_TASK)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_jt_desired: task is not a JointTask");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const double* G = ctx->h_params.task[task].law_goals;
	const size_t k0 = ctx->cfg[task].task_dof;
	int rc;
	if ((rc = fetch_rows(ctx, G, 0, k0, q))) return rc;
	if ((rc = fetch_rows(ctx, G, k0, k0, dq))) return rc;
	return fetch_rows(ctx, G, 2 * k0, k0, ddq);
}
extern "C" int sai2b_get_mft_desired(sai2b_ctx* ctx, int task, double* pos, double* rot, double* lin_vel, double* ang_vel,
									 double* lin_acc, double* ang_acc) {
	int rc = mft_task_check(ctx, task, "sai2b_get_mft_desired");
	if (rc) return rc;
	const double* G = ctx->h_params.task[task].law_goals;
	if ((rc = fetch_rows(ctx, G, sai2b::MFT_GOAL_POS, 3, pos))) return rc;
	if ((rc = fetch_rows(ctx, G, sai2b::MFT_GOAL_ROT, 9, rot))) return rc;
	if ((rc = fetch_rows(ctx, G, sai2b::MFT_GOAL_LIN_VEL, 3, lin_vel))) return rc;
	if ((rc = fetch_rows(ctx, G, sai2b::MFT_GOAL_ANG_VEL, 3, ang_vel))) return rc;
	if ((rc = fetch_rows(ctx, G, sai2b::MFT_GOAL_LIN_ACC, 3, lin_acc))) return rc;
	return fetch_rows(ctx, G, sai2b::MFT_GOAL_ANG_ACC, 3, ang_acc);
}
extern "C" int sai2b_get_otg_status(sai2b_ctx* ctx, int task, double* goal_reached, double* result) {
	if (!ctx || task < 0 || task >= ctx->T) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_otg_status: bad arguments");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = flush_update(ctx);
	if (rc) return rc;
	const double* S = ctx->h_params.task[task].otg_state;
	if ((rc = fetch_rows(ctx, S, sai2b::OTG_GOAL_REACHED, 1, goal_reached))) return rc;
	return fetch_rows(ctx, S, sai2b::OTG_RESULT, 1, result);
}

extern "C" int sai2b_get_model(sai2b_ctx* ctx, int task, double* M, double* J, double* pos, double* rot) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "null ctx");
	if (int rc_ = flush_update(ctx)) return rc_;
	int rc;
	if ((rc = fetch_dbg(ctx, M, ctx->h_params.dbg_M, N * N))) return rc;
	if (!J && !pos && !rot) return SAI2B_OK;
	if ((rc = mft_task_check(ctx, task, "sai2b_get_model"))) return rc;
	const DevTask& d = ctx->h_params.task[task];
	const size_t B = ctx->B;
	if ((rc = fetch_dbg(ctx, J, d.dbg_J, 6 * N))) return rc;
	if ((rc = fetch_dbg(ctx, pos, d.dbg_pose, 3))) return rc;
	return fetch_dbg(ctx, rot, d.dbg_pose ? d.dbg_pose + 3 * B : nullptr, 9);
}

// Bench bookkeeping: run `steps` fused ticks with HIP events around EACH kernel launch of the tick on
// the ctx stream and return the average duration per launch in milliseconds: first kernel of the tick
// (the SVD-free kernel when the hierarchy is eligible, else the generic kernel) and, when there is
// one, the generic kernel over its work list behind it (0 otherwise). In the self form (tick_self_kernel) the tick is one
// kernel: while it declines nothing, that kernel is the first figure and the second is 0. When the last tick declined robots,
// the first figure is the SVD-free kernel by itself, as in the two-launch form, and the second what the self kernel takes
// beyond it, which is what serving those robots inside the launch adds to a step.
extern "C" int sai2b_profile_tick(sai2b_ctx* ctx, int steps, double* first_ms, double* second_ms) {
	if (!ctx || steps < 1) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_profile_tick: bad arguments");
	if (int rc_ = flush_update(ctx)) return rc_;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = upload_params(ctx);
	if (rc) return rc;
	// (the kernel the ticks are running now)
	const TickForm form = sai2b::tick_form(ctx->route, ctx->sw, route_kinds(ctx), ctx->baked_model, ctx->h_params.payload != nullptr);
	const bool self = form.self && !ctx->introspection;
	int declined = 0;
	if (self) {
		HIP_TRY(ctx, hipMemcpyAsync(&declined, ctx->fb.count(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	const bool two = form.fast != 0 && !ctx->introspection && (!self || declined > 0);
	TickForm alone = form;	// the SVD-free kernel by itself
	alone.self = false;
	// ONE event pair around `steps` back-to-back launches (an event pair per launch costs ~4 us of its own, which made
	// the two parts add up to more than the step): first the first kernel alone, then the sequence of a tick. The
	// second figure is what the work-list pass adds to a step, so the two sum to the step by construction.
	hipEvent_t e0, e1;
	HIP_TRY(ctx, hipEventCreate(&e0));
	HIP_TRY(ctx, hipEventCreate(&e1));
	double part_ms[2] = {0, 0};
	for (int phase = 0; phase < (two ? 2 : 1); phase++) {
		for (int rep = 0; rep < 2; rep++) {	 // (the first repetition warms the sequence up)
			HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
			for (int s = 0; s < steps; s++) {
				if (two || self) ctx->fb.parity ^= 1;
				if (sai2b::launch_tick_part(ctrl_params(ctx), ctx->B, (two && phase == 0) ? alone : form, ctx->introspection, 0, ctx->fb,
											sai2b::generic_lanes(ctx->sw, ctx->B, !two), ctx->stream))
					return set_error(ctx, SAI2B_RUNTIME_ERROR, "tick launch failed");
				if (phase == 1 && !self && sai2b::launch_tick_part(ctrl_params(ctx), ctx->B, form, false, 1, ctx->fb, sai2b::generic_lanes(ctx->sw, ctx->B, false), ctx->stream))
					return set_error(ctx, SAI2B_RUNTIME_ERROR, "tick launch failed");
			}
			HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
			HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			float ms = 0;
			HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
			part_ms[phase] = ms / steps;
		}
	}
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	ctx->launches += (two ? (self ? 4 : 6) : 2) * (long long)steps;
	ctx->ticks += (two ? 4 : 2) * (long long)steps * ctx->B;
	if (first_ms) *first_ms = part_ms[0];
	if (second_ms) *second_ms = two ? std::max(0.0, part_ms[1] - part_ms[0]) : 0.0;
	return SAI2B_OK;
}

extern "C" int sai2b_get_fallback_count(sai2b_ctx* ctx, int* robots) {
	if (!ctx || !robots) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_fallback_count: bad arguments");
	if (int rc_ = flush_update(ctx)) return rc_;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (ctx->last_call_task) {	// a TemplateTask call came last: its own work list
		if (ctx->last_call_task == 2) {
			*robots = ctx->B;
			return SAI2B_OK;
		}
		HIP_TRY(ctx, hipMemcpyAsync(robots, ctx->tk.count(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		return SAI2B_OK;
	}
	if (ctx->route.last_generic_only) {	// no SVD-free kernel ran in front: every robot took the generic kernel
		*robots = ctx->B;
		return SAI2B_OK;
	}
	HIP_TRY(ctx, hipMemcpyAsync(robots, ctx->fb.count(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return SAI2B_OK;
}

extern "C" int sai2b_get_worklist_state(const sai2b_ctx* ctx, int* last_seen, int* pending, int* form, int* wmax) {
	if (!ctx) return SAI2B_INVALID_ARGUMENT;
	if (last_seen) *last_seen = ctx->route.last_seen;
	if (pending) *pending = ctx->route.pending();
	if (form) *form = ctx->route.last_form;
	if (wmax) *wmax = ctx->route.last_wmax;
	return SAI2B_OK;
}

extern "C" int sai2b_device_count(void) {
	int n = 0;
	return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int sai2b_counters(const sai2b_ctx* ctx, long long* launches, long long* ticks) {
	if (!ctx) return SAI2B_INVALID_ARGUMENT;
	if (launches) *launches = ctx->launches;
	if (ticks) *ticks = ctx->ticks;
	return SAI2B_OK;
}

// ------------------------------------------------------------------------------------------------
// snapshot banks (include/sai2b.h "snapshot banks"; layout: sai2b_snapshot_layout.h; kernels: sai2b_snapshot.hip)
// ------------------------------------------------------------------------------------------------
static_assert(sai2b::SNAP_JOINT_ROWS == sai2b::JOINT_ROWS && sai2b::SNAP_JOINT_STATUS_ROWS == sai2b::JOINT_STATUS_ROWS &&
				  sai2b::SNAP_WRENCH_MOTION_ROWS + 1 == sai2b::WRENCH_ROWS && 6 + N == sai2b::WRENCH_STATUS_ROWS &&
				  sai2b::MFT_STATE_ROWS == 12 + 3 * N && sai2b::SNAP_HW_SENSOR_ROWS == sai2b::HW_SENSOR_ROWS &&
				  sai2b::SNAP_HW_MAX_DEPTH == sai2b::HW_MAX_DELAY && sai2b::HW_FILTER_ROWS == N + 6 && sai2b::HW_ACT_ROWS == 1 + 3 * N &&
				  sai2b::JS_ROWS == 1 + 5 * N,
			  "sai2b_snapshot_layout.h and the kernels disagree about a buffer's rows");

namespace {
struct SnapBlobHeader {
	char magic[8];	// "SAI2BSNP"
	int version, capacity, words, rows;
	unsigned long long fingerprint;
	sai2b::SnapDesc desc;
	char pad[SAI2B_SNAPSHOT_HEADER_BYTES - 8 - 16 - 8 - sizeof(sai2b::SnapDesc)];
};
static_assert(sizeof(SnapBlobHeader) == SAI2B_SNAPSHOT_HEADER_BYTES, "blob header");
}  // namespace

struct sai2b_snapshot_bank {
	int dof_tag = N;  // FIRST member, as in sai2b_ctx: sai2b_dispatch.cpp routes by it
	sai2b_ctx* owner = nullptr;
	int device = 0, capacity = 0;
	sai2b::SnapDesc desc;
	sai2b::SnapLayout layout;
	char* data = nullptr;			 // [words][capacity] 4-byte words
	unsigned char* valid = nullptr;	 // [capacity]
	sai2b::SnapDevBlock* table = nullptr;
	hipEvent_t last = nullptr;	// behind the last save / load
	size_t data_bytes() const { return (size_t)layout.words * 4 * (size_t)capacity; }
};

// the context as sai2b_snapshot_layout.h sees it; what the chosen groups do not read stays zero
static sai2b::SnapDesc snapshot_describe(const sai2b_ctx* ctx, int what) {
	sai2b::SnapDesc d;
	std::memset(&d, 0, sizeof(d));
	d.dof = N, d.n_tasks = ctx->T, d.what = what;
	const bool epi = what & SAI2B_SNAP_EPISODE, env = what & SAI2B_SNAP_ENVIRONMENT;
	for (int t = 0; t < ctx->T && epi; t++) {
		const DevTask& k = ctx->h_params.task[t];
		d.task[t].kind = k.type, d.task[t].k0 = k.k0;
		d.task[t].otg_mode = k.otg_on ? (k.otg_jerk ? 2 : 1) : 0;
		d.task[t].otg3 = k.otg3_traj != nullptr, d.task[t].popc = k.popc_f != nullptr, d.task[t].nprec = ctx->tio[t].Nprec != nullptr;
	}
	d.steps = epi && ctx->obs_steps != nullptr;
	d.contact = ctx->contact_rows != nullptr && ctx->h_params.contact_status != nullptr;
	d.joint = ctx->joint_rows != nullptr && ctx->joint_status != nullptr;
	d.wrench = ctx->wrench_rows != nullptr && ctx->wrench_status != nullptr;
	d.payload = env && ctx->payload_rows[0] != nullptr, d.plant_payload = env && ctx->payload_rows[1] != nullptr;
	// the hardware's buffers exist from the first sai2b_set_hardware on; the history's depth is that of the last one
	d.hardware = ctx->hw_clock != nullptr;
	d.hardware_depth = d.hardware && epi ? ctx->hw_cfg.max_delay : 0;
	// the reward's accumulators exist from the first sai2b_set_reward on
	d.reward = epi && ctx->rew_state != nullptr;
	// the sampler's episode counters exist from the first sai2b_set_reset_sampler on
	d.reset_sampler = epi && ctx->rs_state != nullptr;
	// the environment sampler's counters and sample rows exist from the first sai2b_set_env_sampler on; the rows are those of the last one
	d.env_sampler = ctx->es_counter != nullptr ? 1 + ctx->es_lay.total : 0;
	// the joint sensors' buffers exist from the first sai2b_set_joint_sensor on; the history's depth is that of the last one
	d.joint_sensor = ctx->js_clock != nullptr;
	d.joint_sensor_depth = d.joint_sensor && epi ? ctx->js_cfg.max_delay : 0;
	return d;
}

// where a block of the table lives in the context
static void* snapshot_block_base(sai2b_ctx* ctx, const sai2b::SnapRow& r) {
	using namespace sai2b;
	const size_t B = ctx->B;
	DevTask* k = r.task >= 0 ? &ctx->h_params.task[r.task] : nullptr;
	switch (r.block) {
		case SNAP_Q: return ctx->q;
		case SNAP_DQ: return ctx->dq;
		case SNAP_TAU: return ctx->tau;
		case SNAP_Q_POSE: return ctx->q_pose;
		case SNAP_GOALS: return k->goals;
		case SNAP_SENSED: return k->sensed;
		case SNAP_STATE: return k->state;
		case SNAP_ISTATE: return k->istate;
		case SNAP_OTG_DESIRED: return k->otg_desired;
		case SNAP_OTG_STATE: return k->otg_state;
		case SNAP_OTG3_TRAJ: return k->otg3_traj;
		case SNAP_POPC_F: return k->popc_f;
		case SNAP_POPC_I: return k->popc_i;
		case SNAP_POPC_Q: return k->popc_q;
		case SNAP_NPREC: return ctx->tio[r.task].Nprec;
		case SNAP_EPISODE_STEP: return ctx->obs_steps;
		case SNAP_WRENCH_REMAINING: return ctx->wrench_rows + (size_t)SNAP_WRENCH_MOTION_ROWS * B;
		case SNAP_CONTACT_STATUS: return ctx->h_params.contact_status;
		case SNAP_JOINT_STATUS: return ctx->joint_status;
		case SNAP_WRENCH_STATUS: return ctx->wrench_status;
		case SNAP_PAYLOAD: return ctx->payload_rows[0];
		case SNAP_PLANT_PAYLOAD: return ctx->payload_rows[1];
		case SNAP_CONTACT: return ctx->contact_rows;
		case SNAP_JOINT: return ctx->joint_rows;
		case SNAP_WRENCH: return ctx->wrench_rows;
		case SNAP_HW_HISTORY: return ctx->hw_history;
		case SNAP_HW_FILTER: return ctx->hw_filter;
		case SNAP_HW_APPLIED: return ctx->hw_applied;
		case SNAP_HW_CLOCK: return ctx->hw_clock;
		case SNAP_HW_ACTUATOR: return ctx->hw_act;
		case SNAP_HW_SENSOR: return ctx->hw_sensor;
		case SNAP_REWARD_STATE: return ctx->rew_state;
		case SNAP_REWARD_EPISODE: return ctx->rew_episode;
		case SNAP_RS_EPISODE: return ctx->rs_state;
		case SNAP_ES_COUNTER: return ctx->es_counter;
		case SNAP_ES_SAMPLE: return ctx->es_sample;
		case SNAP_JS_Q: return ctx->js_qm;
		case SNAP_JS_DQ: return ctx->js_dqm;
		case SNAP_JS_PREV: return ctx->js_prev;
		case SNAP_JS_FILTER: return ctx->js_filter;
		case SNAP_JS_HISTORY: return ctx->js_history;
		case SNAP_JS_CLOCK: return ctx->js_clock;
		case SNAP_JS_ROWS: return ctx->js_rows;
		default: return nullptr;
	}
}

static bool snapshot_what_ok(int what) { return what > 0 && (what & ~(SAI2B_SNAP_EPISODE | SAI2B_SNAP_ENVIRONMENT)) == 0; }

extern "C" int sai2b_snapshot_words(sai2b_ctx* ctx, int what) {
	if (!ctx || !snapshot_what_ok(what)) {
		set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_words: bad arguments");
		return -1;
	}
	return sai2b::snapshot_layout(snapshot_describe(ctx, what)).words;
}

extern "C" int sai2b_snapshot_layout(sai2b_ctx* ctx, int what, int* table5, int max_rows) {
	if (!ctx || !snapshot_what_ok(what) || (max_rows > 0 && !table5)) {
		set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_layout: bad arguments");
		return -1;
	}
	const sai2b::SnapLayout L = sai2b::snapshot_layout(snapshot_describe(ctx, what));
	for (int i = 0; i < L.n && i < max_rows; i++) {
		const sai2b::SnapRow& r = L.row[i];
		const int v[5] = {r.block, r.task, r.rows, r.elem_bytes, r.first_word};
		std::memcpy(table5 + 5 * i, v, sizeof(v));
	}
	return L.n;
}

extern "C" void sai2b_snapshot_bank_destroy(sai2b_snapshot_bank* bank) {
	if (!bank) return;
	(void)hipSetDevice(bank->device);
	if (bank->last) {
		(void)hipEventSynchronize(bank->last);
		(void)hipEventDestroy(bank->last);
	}
	if (bank->data) (void)hipFree(bank->data);
	if (bank->valid) (void)hipFree(bank->valid);
	if (bank->table) (void)hipFree(bank->table);
	delete bank;
}

extern "C" int sai2b_snapshot_bank_create(sai2b_ctx* ctx, int capacity, int what, sai2b_snapshot_bank** out) {
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_bank_create: null ctx");
	if (!out || capacity < 1 || !snapshot_what_ok(what))
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_bank_create: capacity must be >= 1 and what a combination of SAI2B_SNAP_*");
	*out = nullptr;
	int rc = flush_update(ctx);
	if (rc) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!ctx->snap_counts) {
		if ((rc = dev_alloc(ctx, &ctx->snap_counts, 4))) return rc;
		HIP_TRY(ctx, hipHostMalloc((void**)&ctx->snap_report, 3 * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
		ctx->snap_report[0] = ctx->snap_report[1] = ctx->snap_report[2] = 0;
		HIP_TRY(ctx, hipHostGetDevicePointer((void**)&ctx->snap_report_dev, ctx->snap_report, 0));
	}
	sai2b_snapshot_bank* bank = new sai2b_snapshot_bank();
	bank->owner = ctx, bank->device = ctx->device, bank->capacity = capacity;
	bank->desc = snapshot_describe(ctx, what);
	bank->layout = sai2b::snapshot_layout(bank->desc);
	std::vector<sai2b::SnapDevBlock> table(bank->layout.n);
	for (int i = 0; i < bank->layout.n; i++) {
		const sai2b::SnapRow& r = bank->layout.row[i];
		table[i] = sai2b::SnapDevBlock{snapshot_block_base(ctx, r), r.rows, r.elem_bytes, r.first_word, r.first_row, r.block == sai2b::SNAP_Q_POSE, 0};
	}
	auto fail = [&](hipError_t e, const char* what_failed) {
		sai2b_snapshot_bank_destroy(bank);
		return set_error(ctx, SAI2B_RUNTIME_ERROR, std::string("sai2b_snapshot_bank_create: ") + what_failed + ": " + hipGetErrorString(e));
	};
	hipError_t e;
	if ((e = hipMalloc((void**)&bank->data, std::max<size_t>(bank->data_bytes(), 8))) != hipSuccess) return fail(e, "hipMalloc of the bank");
	if ((e = hipMalloc((void**)&bank->valid, (size_t)capacity)) != hipSuccess) return fail(e, "hipMalloc of the valid bytes");
	if ((e = hipMalloc((void**)&bank->table, std::max<size_t>(table.size(), 1) * sizeof(sai2b::SnapDevBlock))) != hipSuccess)
		return fail(e, "hipMalloc of the row table");
	if ((e = hipEventCreateWithFlags(&bank->last, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
	if ((e = hipMemsetAsync(bank->data, 0, std::max<size_t>(bank->data_bytes(), 8), ctx->stream)) != hipSuccess) return fail(e, "hipMemset");
	if ((e = hipMemsetAsync(bank->valid, 0, (size_t)capacity, ctx->stream)) != hipSuccess) return fail(e, "hipMemset");
	if (!table.empty() &&
		(e = hipMemcpyAsync(bank->table, table.data(), table.size() * sizeof(sai2b::SnapDevBlock), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
		return fail(e, "upload of the row table");
	if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail(e, "hipStreamSynchronize");
	*out = bank;
	return SAI2B_OK;
}

// save (true) / load (false): one launch of snapshot_kernel
static int snapshot_move(sai2b_ctx* ctx, sai2b_snapshot_bank* bank, const int* slot, const unsigned char* mask, int on_device, bool save) {
	const std::string fn = save ? "sai2b_snapshot_save" : "sai2b_snapshot_load";
	if (!ctx) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, fn + ": null ctx");
	if (!bank) return set_error(ctx, SAI2B_INVALID_ARGUMENT, fn + ": null bank");
	if (bank->owner != ctx) return set_error(ctx, SAI2B_INVALID_ARGUMENT, fn + ": the bank was created for another context");
	int rc = flush_update(ctx);
	if (rc) return rc;
	const sai2b::SnapDesc now = snapshot_describe(ctx, bank->desc.what);
	char diff[160] = "";
	if (sai2b::snapshot_first_difference(bank->desc, now, diff, sizeof(diff)))
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, fn + ": the context's layout has changed since the bank was created, first at " + diff);
	if (!slot && bank->capacity < ctx->B) return set_error(ctx, SAI2B_INVALID_ARGUMENT, fn + ": slot NULL (slot b for robot b) needs capacity >= batch");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t B = ctx->B;
	const int* d_slot = slot;
	const unsigned char* d_mask = mask;
	if (on_device) {
		if ((slot || mask) && (rc = caller_before_read(ctx))) return rc;
	} else if (slot || mask) {
		if (mask) {
			if (!ctx->reset_mask && (rc = dev_alloc(ctx, &ctx->reset_mask, B))) return rc;
			HIP_TRY(ctx, hipMemcpyAsync(ctx->reset_mask, mask, B, hipMemcpyHostToDevice, ctx->stream));
			d_mask = ctx->reset_mask;
		}
		if (slot) {
			if (!ctx->snap_slot && (rc = dev_alloc(ctx, &ctx->snap_slot, B))) return rc;
			HIP_TRY(ctx, hipMemcpyAsync(ctx->snap_slot, slot, B * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
			d_slot = ctx->snap_slot;
		}
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // pageable host memory may be reused by the caller
	}
	sai2b::SnapArgs a;
	a.table = bank->table, a.n_blocks = bank->layout.n, a.total_rows = bank->layout.rows;
	a.B = ctx->B, a.capacity = bank->capacity, a.dof = N;
	if (++ctx->snap_stamp == 0) ctx->snap_stamp = 1;
	a.stamp = ctx->snap_stamp;
	a.bank = bank->data, a.valid = bank->valid, a.slot = d_slot, a.mask = d_mask;
	a.counts = ctx->snap_counts, a.report = ctx->snap_report_dev;
	const bool episode = bank->desc.what & SAI2B_SNAP_EPISODE;
	// q_is_pose is one flag for the batch. A save stores the cached pose from wherever it lives. A load puts a loaded robot's pose
	// into q_pose, so the flag ends for the batch: the robots the call leaves alone get q_pose := q in the same launch.
	if (save && ctx->q_is_pose) a.pose_src = ctrl_q(ctx);
	if (!save && episode && ctx->q_is_pose) a.keep_pose_q = ctrl_q(ctx), a.keep_pose_dst = ctx->q_pose;
	if (sai2b::launch_snapshot(a, save, ctx->stream)) return set_error(ctx, SAI2B_RUNTIME_ERROR, fn + ": launch failed");
	ctx->launches++;
	HIP_TRY(ctx, hipEventRecord(bank->last, ctx->stream));
	if (!save) {
		if (episode) ctx->q_is_pose = false;
		// as reset_subset: batch-wide and conservative
		ctx->goals_dirty = ~0u;
		ctx->goals_epoch++, ctx->otg_all_idle = false;
		ctx->models_fresh = false;
		for (int t = 0; t < ctx->T; t++) ctx->tio[t].model_fresh = false;
	}
	return (on_device && (slot || mask)) ? caller_after_read(ctx) : SAI2B_OK;
}

extern "C" int sai2b_snapshot_save(sai2b_ctx* ctx, sai2b_snapshot_bank* bank, const int* slot, const unsigned char* mask, int on_device) {
	return snapshot_move(ctx, bank, slot, mask, on_device, true);
}
extern "C" int sai2b_snapshot_load(sai2b_ctx* ctx, sai2b_snapshot_bank* bank, const int* slot, const unsigned char* mask, int on_device) {
	return snapshot_move(ctx, bank, slot, mask, on_device, false);
}

extern "C" int sai2b_get_snapshot_counts(sai2b_ctx* ctx, int counts[3]) {
	if (!ctx || !counts) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_get_snapshot_counts: bad arguments");
	counts[0] = counts[1] = counts[2] = 0;
	if (!ctx->snap_stamp) return SAI2B_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	for (int k = 0; k < 3; k++) {
		const unsigned long long w = __atomic_load_n(ctx->snap_report + k, __ATOMIC_ACQUIRE);
		if ((unsigned)(w >> 32) != ctx->snap_stamp)
			return set_error(ctx, SAI2B_RUNTIME_ERROR, "sai2b_get_snapshot_counts: the counts of the last call have not arrived");
		counts[k] = (int)(unsigned)w;
	}
	return SAI2B_OK;
}

extern "C" size_t sai2b_snapshot_export_size(const sai2b_snapshot_bank* bank) {
	return bank ? SAI2B_SNAPSHOT_HEADER_BYTES + bank->data_bytes() + (size_t)bank->capacity : 0;
}

extern "C" int sai2b_snapshot_export(sai2b_snapshot_bank* bank, void* host_blob, size_t size) {
	if (!bank) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_export: null bank");
	sai2b_ctx* ctx = nullptr;  // (the bank may outlive nothing, but it never dereferences its context here)
	if (!host_blob || size < sai2b_snapshot_export_size(bank))
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_export: the blob is smaller than sai2b_snapshot_export_size");
	HIP_TRY(ctx, hipSetDevice(bank->device));
	HIP_TRY(ctx, hipEventSynchronize(bank->last));
	SnapBlobHeader h;
	std::memset(&h, 0, sizeof(h));
	std::memcpy(h.magic, "SAI2BSNP", 8);
	h.version = 1, h.capacity = bank->capacity, h.words = bank->layout.words, h.rows = bank->layout.rows;
	h.fingerprint = bank->layout.fingerprint, h.desc = bank->desc;
	char* blob = (char*)host_blob;
	std::memcpy(blob, &h, sizeof(h));
	if (bank->data_bytes()) HIP_TRY(ctx, hipMemcpy(blob + sizeof(h), bank->data, bank->data_bytes(), hipMemcpyDeviceToHost));
	HIP_TRY(ctx, hipMemcpy(blob + sizeof(h) + bank->data_bytes(), bank->valid, (size_t)bank->capacity, hipMemcpyDeviceToHost));
	return SAI2B_OK;
}

extern "C" int sai2b_snapshot_import(sai2b_snapshot_bank* bank, const void* host_blob, size_t size) {
	if (!bank) return set_error(nullptr, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_import: null bank");
	sai2b_ctx* ctx = nullptr;
	if (!host_blob || size < sizeof(SnapBlobHeader)) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_import: the blob is shorter than its header");
	SnapBlobHeader h;
	std::memcpy(&h, host_blob, sizeof(h));
	if (std::memcmp(h.magic, "SAI2BSNP", 8) != 0 || h.version != 1)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_import: not a snapshot blob of this library version");
	char diff[160] = "";
	if (sai2b::snapshot_first_difference(h.desc, bank->desc, diff, sizeof(diff)) || h.fingerprint != bank->layout.fingerprint)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, std::string("sai2b_snapshot_import: the blob's layout is not the bank's, first at ") +
														  (h.fingerprint != bank->layout.fingerprint && !diff[0] ? "block q: fingerprint" : diff));
	if (h.capacity != bank->capacity || h.words != bank->layout.words)
		return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_import: the blob's capacity is not the bank's");
	if (size < sai2b_snapshot_export_size(bank)) return set_error(ctx, SAI2B_INVALID_ARGUMENT, "sai2b_snapshot_import: the blob is truncated");
	HIP_TRY(ctx, hipSetDevice(bank->device));
	HIP_TRY(ctx, hipEventSynchronize(bank->last));
	const char* blob = (const char*)host_blob;
	if (bank->data_bytes()) HIP_TRY(ctx, hipMemcpy(bank->data, blob + sizeof(h), bank->data_bytes(), hipMemcpyHostToDevice));
	HIP_TRY(ctx, hipMemcpy(bank->valid, blob + sizeof(h) + bank->data_bytes(), (size_t)bank->capacity, hipMemcpyHostToDevice));
	HIP_TRY(ctx, hipDeviceSynchronize());
	return SAI2B_OK;
}

// sai2b_launch.h — launch entry points shared by the kernel files and sai2b_host.cpp. Every launcher returns 0 when
// all its kernels were launched and non-zero otherwise.
#pragma once
#include <hip/hip_runtime.h>

#include "sai2b_body_contact_law.h"  // BcGeom
#include "sai2b_collision_law.h"  // ColLaw
#include "sai2b_env_draw.h"  // EnvDraw
#include "sai2b_ik_law.h"  // IkLaw
#include "sai2b_params.h"
#include "sai2b_tick_policy.h"  // TickForm, TickCall

namespace sai2b {

// Robots a first kernel declined, compacted for the generic kernel behind it. counts: two counters, zero before the
// first launch, alternating between launches (`parity`): a launch fills [parity] and clears [1 - parity] for the next
// one. list: [B] robot indices. The tick's list has two more counters at [2..3], alternating alike: robots that went
// through the in-lane singular branch of tick_cert_kernel. The generators' list (sai2b_otg.hip) is
// counts [2][SAI2B_MAX_TASKS] + 2 (non-idle robots of a tick, alternating) and list [SAI2B_MAX_TASKS][B].
// The tick's list also has counts[4..5], alternating alike: the largest number of robots one wavefront of tick_fast_kernel /
// tick_self_kernel declined.
// report: the mapped host words through which the pass over the tick's list tells the host the list's counts (device address;
// three 8-byte words, see tick_group_kernel). The tick's list alone has them.
struct WorkList {
	int* counts = nullptr;
	int* list = nullptr;
	int parity = 0;
	unsigned long long* report = nullptr;
	int* count() const { return counts + parity; }
	int* took() const { return counts + 2 + parity; }
};

inline int launch_result() { return hipGetLastError() == hipSuccess ? 0 : 1; }

// the SVD-free kernel of `form` (when the call is a plain torque tick) with the generic kernel over its work list
// behind it, or the generic kernel for the whole batch
int launch_tick(const DevParams* d_params, int B, const TickForm& form, const TickCall& call, const WorkList& fb, hipStream_t stream);
// generic tick with a robot spread over `lanes` = 16 or 8 lanes (sai2b_group.hip); fb_count / fb_list as tick_kernel
// report != NULL (with a work list): workgroup 0 writes {stamp << 32 | count, stamp << 32 | fb_count[2], stamp << 32 | fb_count[4]}
// there, system scope
int launch_tick_group(const DevParams* d_params, int B, int lanes, bool range_only, bool commit_sh, bool with_comp, bool do_torque,
					  const int* fb_count, const int* fb_list, hipStream_t stream, unsigned long long* report = nullptr, unsigned stamp = 0);
// the tick of form.self in one launch (sai2b_self.hip); stamp != 0: a one-lane launch behind it writes fb.report as above
int launch_tick_self(const DevParams* d_params, int B, const TickForm& form, bool with_comp, const WorkList& fb, unsigned stamp,
					 hipStream_t stream);
// the SVD-free tick for general hierarchies (sai2b_cert.hip, form.fast >= 3): fills the work list like the fast kernels
int launch_tick_cert(const DevParams* d_params, int B, const TickForm& form, bool with_comp, const WorkList& fb, hipStream_t stream);
// the range pass ahead of the trajectory generators for certified robots (sai2b_cert.hip: range_cert_kernel); the rest
// of the batch goes to rg for launch_tick_group(..., range_only = true, ...). max_rows: as TickForm::fast - 3
int launch_range_cert(const DevParams* d_params, int B, int max_rows, bool payload, bool inlane_singular, const WorkList& rg,
					  hipStream_t stream);
int launch_range_pass(const DevParams* d_params, int B, bool debug, bool with_comp, int group, hipStream_t stream);
// only_task < 0: every task (RobotController::reinitializeTasks); else TemplateTask::reInitializeTask of that one
int launch_reinit(const DevParams* d_params, int B, int only_task, hipStream_t stream);
// one task on its own (TemplateTask.h:42-88): model update (do_torque = false) or the task's torques (do_torque = true)
// under a caller-supplied N_prec ([N*N][B], NULL = identity) and tau_prec ([N][B], NULL = the no-argument
// computeTorques()); N_out / Ntot_out [N*N][B]: the task's nullspace and N * N_prec; tau_out [N][B]
int launch_task_group(const DevParams* d_params, int B, int lanes, int task, const double* Nprec_in, const double* tau_prec, double* tau_out,
					  double* N_out, double* Ntot_out, bool commit_sh, bool do_torque, const int* tk_count, const int* tk_list,
					  hipStream_t stream);
int launch_task(const DevParams* d_params, int B, int task, const double* Nprec_in, const double* tau_prec, double* tau_out, double* N_out,
				double* Ntot_out, bool commit_sh, bool do_torque, const int* tk_count, const int* tk_list, hipStream_t stream);
// the same calls through the whitened cascade (sai2b_cert.hip: task_cert_kernel); robots it declines are appended to tk
// for launch_task(..., tk.count(), tk.list) behind it. max_rows: rows of the task (<= 3: the small instantiation)
int launch_task_cert(const DevParams* d_params, int B, int task, int max_rows, bool payload, bool inlane_singular, const double* Nprec_in,
					 const double* tau_prec, double* tau_out, double* N_out, double* Ntot_out, bool commit_sh, bool do_torque,
					 const WorkList& tk, hipStream_t stream);
// one kernel of a full tick (commit, compensation, torques) on its own, for per-kernel timing: part 0 = first kernel,
// part 1 = the generic kernel over the work list of the SVD-free one
int launch_tick_part(const DevParams* d_params, int B, const TickForm& form, bool debug, int part, const WorkList& fb, int group,
					 hipStream_t stream);
// internal OTG (sai2b_otg.hip): one update of every enabled generator; (re)initialisation (modes in the kernel's comment)
// task_mask bit t: advance task t's generator (all enabled ones: ~0)
int launch_otg(const DevParams* d_params, int B, const WorkList& otg, int clean_mask, int task_mask, int jerk_mask, hipStream_t stream);
// q_pose: [N][B] joint positions the tasks' cached poses correspond to (read in mode 1 only)
int launch_otg_reinit(const DevParams* d_params, int B, int only_task, int mode, const double* q_pose, hipStream_t stream);
// the masked robots' reinit + OTG reinit (mode 0) in one launch (sai2b_otg.hip: reset_subset_kernel). mask [B] device bytes;
// q_new / dq_new [N][B] device rows or NULL; q_state / dq_state / q_pose: the ctx buffers; flags: RESET_*
enum { RESET_EPISODE = 1, RESET_KEEP_POSE = 2 };
int launch_reset_subset(const DevParams* d_params, int B, const unsigned char* mask, const double* q_new, const double* dq_new, double* q_state,
						double* dq_state, double* q_pose, int only_task, int flags, hipStream_t stream);
// force / motion space re-parametrisation of MotionForceTask `task` at run time (flags in the kernel's comment)
int launch_mft_reparam(const DevParams* d_params, int B, int task, int flags, const double* q_pose, hipStream_t stream);
// joint dynamics of the plant (sai2b_set_joint_dynamics, sai2b_sim.hip: sim_joint_kernel): the kernel's own parameter block,
// passed by value as a kernel argument like ObsParams; DevParams is not touched by the feature.
constexpr int JOINT_ROWS = 6, JOINT_STATUS_ROWS = 3, JOINT_COUNTS = 2;
enum { JOINT_ARMATURE = 0, JOINT_DAMPING, JOINT_FRICTION, JOINT_TORQUE_LIMIT, JOINT_LOWER, JOINT_UPPER };
struct JointParams {
	const double* rows = nullptr;  // [JOINT_ROWS][N][B]
	double* status = nullptr;	   // [JOINT_STATUS_ROWS][N][B]: applied, stop and dissipative torque
	int* counts = nullptr;		   // [JOINT_COUNTS]: robots saturated, robots at a stop; zeroed by the caller ahead of the launch
	double stop_k[N] = {}, stop_c[N] = {}, v_eps[N] = {};
};
// external wrench on a link of the plant (sai2b_set_external_wrench, sai2b_sim.hip: sim_wrench_kernel / sim_joint_wrench_kernel):
// the kernels' own parameter block, passed by value as a kernel argument like JointParams; DevParams is not touched by the feature.
constexpr int WRENCH_ROWS = 7, WRENCH_STATUS_ROWS = 6 + N;
struct WrenchParams {
	double* rows = nullptr;	   // [WRENCH_ROWS][B]: force 3, moment 3, remaining pushed periods (counted down by the kernel)
	double* status = nullptr;  // [WRENCH_STATUS_ROWS][B]: F_w, M_w about x, tx at the final state
	int* count = nullptr;	   // robots pushed; zeroed by the caller ahead of the launch
	int link = 0, frame = 0, sensor_task = -1;
	double point[3] = {};
};
// whole-arm contact of the plant (sai2b_set_body_contact, sai2b_sim.hip: sim_body_kernel): the kernel's own parameter block, passed
// by value as a kernel argument like WrenchParams; DevParams is not touched by the feature. The geometry is the collision
// configuration's, the environment rows are the collision's own buffer, read live.
struct BodyParams {
	BcGeom geom = {};
	const double* env = nullptr;   // [6 P + 4 O][B], or NULL without planes and obstacles
	const double* rows = nullptr;  // [BC_ROWS][B]: stiffness, damping, friction
	double* status = nullptr;	   // [9 + N][B]
	int* counts = nullptr;		   // [BC_COUNTS]; zeroed by the caller ahead of the launch
};
// simulation harness (sai2b_sim.hip): one control period of rigid-body dynamics, state updated in place.
// payload / contact select the instantiation: the plant's payload rows, the contact rows, status and counter of DevParams;
// joint != NULL: sim_joint_kernel (the same two selectors) instead of sim_kernel, dbg_bias must be NULL then;
// wrench != NULL: the forms of either with an external wrench, dbg_bias must be NULL then;
// body != NULL: sim_body_kernel instead of all of them (joint and wrench become its switches), dbg_bias must be NULL then
int launch_sim(const DevParams* d_params, int B, const double* tau, double dt, int substeps, int with_gravity, bool payload, bool contact,
			   const JointParams* joint, const WrenchParams* wrench, const BodyParams* body, double* dbg_bias, double* q_keep, hipStream_t stream);
// observers of a MotionForceTask between ticks: out [68][B] (rows in sai2b_sim.hip: mft_status_kernel)
int launch_mft_status(const DevParams* d_params, int B, int task, double* out, hipStream_t stream);

// sai2b_observe (sai2b_observe.hip: observe_kernel): the kernel's own parameter block, passed by value as a kernel argument
// (batch-uniform, read with scalar loads); DevParams is not touched by the feature. Rows are first rows of the [rows][B]
// output, -1 = block not stored.
constexpr int OBS_GLOBAL_BLOCKS = 6, OBS_TASK_BLOCKS = 4, OBS_COUNTS = SAI2B_DONE_REASONS + 1;
struct ObsParams {
	int blocks = 0, task_mask = 0, task_blocks = 0;	 // what is stored (sai2b_observation_config)
	int criteria = 0, success_mask = 0, force_mask = 0, max_steps = 0;
	int row_global[OBS_GLOBAL_BLOCKS] = {-1, -1, -1, -1, -1, -1};  // Q, DQ, TAU, LIMIT_MARGIN, EPISODE_STEP, CONTACT
	int row_task[SAI2B_MAX_TASKS] = {-1, -1, -1, -1};			   // first row of task t's blocks (stored in flag order)
	double pos_tol = 0, ori_tol = 0, limit_margin = 0, max_force = 0;
	double max_speed[N] = {};
};
// out [rows][B] or NULL, done [B] bytes or NULL, steps [B] episode counters, counts [OBS_COUNTS] zeroed by the caller on the
// stream ahead of the launch
int launch_observe(const DevParams* d_params, int B, const ObsParams& obs, double* out, unsigned char* done, int* steps, int* counts,
				   hipStream_t stream);

// sai2b_observe_reward (sai2b_observe.hip: observe_reward_kernel, the REWARD instantiation of observe_kernel's body): the reward's
// own parameter block, passed by value beside ObsParams. Rows are rows of the [rows][B] terms output, -1 = term not selected;
// a task's terms stand at row_task[t] + off_task[bit]. row_weight: the weight of every task-term row, by its distance from the
// first task-term row (the order the reward is summed in).
constexpr int REW_TERMS = SAI2B_REWARD_TERMS, REW_TASK_TERMS = SAI2B_REWARD_TASK_TERMS, REW_COUNTS = 2;	 // counts: closed, replaced
constexpr int REW_STATE_ROWS = 3 + N, REW_EPISODE_ROWS = 2;
enum { REW_RET = 0, REW_DISC = 1, REW_LAST_RETURN = 2, REW_TAU_PREV = 3 };	// rows of state; episode: last_length, tau_prev_valid
struct RewParams {
	int terms = 0, task_mask = 0, task_terms = 0;
	int global_rows = 0, task_rows = 0;	 // rows of the global terms, rows of all task terms
	int row_global[REW_TERMS] = {-1, -1, -1, -1, -1, -1};
	int row_task[SAI2B_MAX_TASKS] = {-1, -1, -1, -1};
	int off_task[REW_TASK_TERMS] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
	double weight[REW_TERMS] = {};
	double row_weight[SAI2B_MAX_TASKS * REW_TASK_TERMS] = {};
	double done_value[SAI2B_DONE_REASONS] = {};
	double limit_soft_margin = 0, gamma = 1, nonfinite_reward = 0;
	double pos_scale[SAI2B_MAX_TASKS] = {}, ori_scale[SAI2B_MAX_TASKS] = {}, force_soft_limit[SAI2B_MAX_TASKS] = {};
	double* reward = nullptr;  // [B] or NULL
	double* rows = nullptr;	   // [global_rows + task_rows][B] or NULL
	double* state = nullptr;   // [REW_STATE_ROWS][B]
	int* episode = nullptr;	   // [REW_EPISODE_ROWS][B]
	int* counts = nullptr;	   // [REW_COUNTS], zeroed by the caller on the stream ahead of the launch
};
// as launch_observe, with the reward evaluated in the same launch
int launch_observe_reward(const DevParams* d_params, int B, const ObsParams& obs, const RewParams& rew, double* out, unsigned char* done,
						  int* steps, int* counts, hipStream_t stream);
// the selected robots' ret := 0, disc := 1, tau_prev invalid; mask [B] device bytes
int launch_reward_reset(int B, const unsigned char* mask, double* state, int* episode, hipStream_t stream);

// sai2b_apply_action (sai2b_action.hip: action_kernel): its own parameter block, passed by value as a kernel argument like
// ObsParams; DevParams is not touched by the feature. Per task what sai2b_action_task holds, with the task's first action row.
constexpr int ACT_BLOCKS = 4, ACT_COUNTS = 3;  // counts: rejected, clipped, limited
struct ActTask {
	int mode = 0, blocks = 0, row = -1, reserved = 0;
	double pos_scale[3] = {}, ori_scale = 0, force_scale = 0, moment_scale = 0;
	double pos_lower[3] = {}, pos_upper[3] = {}, max_lead = 0;
	double jt_scale[N] = {}, jt_lower[N] = {}, jt_upper[N] = {};
};
struct ActParams {
	int rows = 0, clip = 0;
	int need_state = 0;	 // some task reads q: DELTA_CURRENT, or a finite lead
	int need_pose = 0;	 // some MotionForceTask reads the current pose: fk() is computed, once for all tasks
	ActTask task[SAI2B_MAX_TASKS];
};
// action [rows][B], mask [B] bytes or NULL, counts [ACT_COUNTS] zeroed by the caller on the stream ahead of the launch
int launch_action(const DevParams* d_params, int B, const ActParams& act, const double* action, const unsigned char* mask, int* counts,
				  hipStream_t stream);

// snapshot banks (sai2b_snapshot_save / sai2b_snapshot_load, sai2b_snapshot.hip: snapshot_kernel): the kernel's own argument
// block, passed by value; DevParams is not read. table: the bank's row table on the device (sai2b_snapshot_layout.h), each block
// with its base pointer in the context.
constexpr int SNAP_CHUNK_ROWS = 32;	 // rows of the table one workgroup moves (the grid's second dimension counts the chunks)
struct SnapDevBlock {
	void* base;	 // [rows][B] elements of elem_bytes in the context
	int rows, elem_bytes, first_word, first_row;
	int pose, reserved;	 // pose: the q_pose block (a save reads SnapArgs::pose_src instead when that is set)
};
struct SnapArgs {
	const SnapDevBlock* table = nullptr;
	int n_blocks = 0, total_rows = 0;
	int B = 0, capacity = 0, dof = 0;
	unsigned stamp = 0;
	char* bank = nullptr;			  // [words][capacity] 4-byte words
	unsigned char* valid = nullptr;	  // [capacity]
	const int* slot = nullptr;		  // [B] or NULL: slot b
	const unsigned char* mask = nullptr;  // [B] or NULL: every robot
	int* counts = nullptr;			  // [4]: moved, out of range, never saved, ticket; zero between launches
	unsigned long long* report = nullptr;  // three mapped host words (device address): stamp << 32 | count
	const double* pose_src = nullptr;	   // save: where the cached pose lives now when that is not q_pose (q while q_is_pose holds)
	const double* keep_pose_q = nullptr;   // load while q_is_pose holds: robots left alone get q_pose := q ...
	double* keep_pose_dst = nullptr;	   // ... here
};
int launch_snapshot(const SnapArgs& args, bool save, hipStream_t stream);

// actuator and force-sensor models around the simulation kernel (sai2b_set_hardware, sai2b_hardware.hip): each kernel has its
// own parameter block, passed by value as a kernel argument like WrenchParams; DevParams is not touched by the feature.
constexpr int HW_MAX_DELAY = 8;					  // SAI2B_MAX_ACTUATION_DELAY
constexpr int HW_ACT_ROWS = 1 + 3 * N;			  // delay, lag coefficient [N], gain [N], noise deviation [N]
constexpr int HW_SENSOR_ROWS = 13;				  // bias 6, noise deviation 6, filter coefficient
constexpr int HW_FILTER_ROWS = N + 6;			  // the lag state f [N], the sensor filter state g [6]
enum { HW_STREAM_ACTUATOR = 0, HW_STREAM_SENSOR = 1 };
struct HwStream {
	unsigned key0 = 0, key1 = 0, first_robot = 0;  // the generator's key (seed low, high) and the global index of robot 0
};
struct ActuateParams {
	const double* rows = nullptr;  // [HW_ACT_ROWS][B]
	const double* command = nullptr;  // [N][B]: the torques the caller commands in this call
	double* history = nullptr;		  // [depth + 1][N][B]
	double* filter = nullptr;		  // [HW_FILTER_ROWS][B]; the kernel touches the first N rows
	double* applied = nullptr;		  // [N][B]: what the simulation kernel receives
	int* clock = nullptr;			  // [2][B]: period n, episode e; the kernel leaves n + 1
	int depth = 0;
	HwStream rng;
};
struct SenseParams {
	const double* rows = nullptr;  // [HW_SENSOR_ROWS][B]
	double* sensed = nullptr;	   // [6][B]: the task's sensed rows, the ideal reading on entry
	double* filter = nullptr;	   // [HW_FILTER_ROWS][B]; the kernel touches the last 6 rows
	const int* clock = nullptr;	   // [2][B] as actuate_kernel left it in this call: the period is clock - 1
	HwStream rng;
};
// joint sensors (sai2b_set_joint_sensor, sai2b_joint_sensor.hip: joint_sense_kernel): the kernel's own parameter block, passed by
// value like SenseParams; DevParams is not read (the controller-side kernels get a copy of it whose q, dq are the measured pair).
constexpr int JS_ROWS = 1 + 5 * N;	// delay; offset, position noise, quantum, velocity noise, velocity filter coefficient [N] each
struct JointSenseParams {
	const double* rows = nullptr;		  // [JS_ROWS][B]
	const double *q = nullptr, *dq = nullptr;  // [N][B]: the truth
	double *q_meas = nullptr, *dq_meas = nullptr;  // [N][B]: the delivered reading
	double *prev = nullptr, *filter = nullptr;	   // [N][B] each: the previous position reading, the velocity filter's state
	double* history = nullptr;			  // [depth + 1][2 N][B]
	int* clock = nullptr;				  // [2][B]: index of the next reading c, episode e
	double* q_pose = nullptr;			  // step: q_meas is saved here first (NULL: not)
	const unsigned char* mask = nullptr;  // seed: [B] bytes or NULL = every robot
	int depth = 0, velocity_mode = 0;
	int next_episode = 0;  // seed: e += 1
	double dt = 0;		   // step: the period of the sai2b_sim_step call
	HwStream rng;
};
// seed: reading 0 of the masked robots, clock := 1; else reading c of every robot, clock := c + 1
int launch_joint_sense(int B, const JointSenseParams& p, bool seed, hipStream_t stream);
int launch_actuate(int B, const ActuateParams& p, hipStream_t stream);
int launch_sense(int B, const SenseParams& p, hipStream_t stream);
// the selected robots' period := 0, episode += 1; mask [B] device bytes
int launch_hardware_reset(int B, const unsigned char* mask, int* clock, hipStream_t stream);

// sai2b_reset_robots_sampled (sai2b_otg.hip: reset_sampled_kernel): launch_reset_subset with RESET_EPISODE for the masked robots,
// their q, dq and goals drawn in the same launch. The sampler's own parameter block, passed by value as a kernel argument like
// ObsParams; DevParams is not touched by the feature. Rows are rows of the [rows][B] per-robot buffer (sai2b_reset_sampler_layout.h).
constexpr int RS_COUNTS = 3;  // robots reset, candidates rejected, robots exhausted
struct RsParams {
	const double* rows = nullptr;  // q_lower, q_upper, dq_sigma, q_nominal [N] each, then the goal rows
	int* episode = nullptr;		   // [B]
	int* tries = nullptr;		   // [B]
	int* counts = nullptr;		   // [RS_COUNTS], zeroed by the caller on the stream ahead of the launch
	HwStream rng;
	int max_tries = 1;
	unsigned goal_tasks = 0, absolute_position = 0;
	int ratio_task = -1, box_task = -1, use_clearance = 0;
	int goal_row[SAI2B_MAX_TASKS] = {-1, -1, -1, -1};  // first goal row of task t, -1: none
	double min_ratio = 0, clearance = 0;
	double box_lower[3] = {}, box_upper[3] = {};
};
// mask [B] device bytes; q_state / dq_state / q_pose: the ctx buffers; flags: RESET_KEEP_POSE or 0 (RESET_EPISODE is implied)
int launch_reset_sampled(const DevParams* d_params, int B, const RsParams& rs, const unsigned char* mask, double* q_state, double* dq_state,
						 double* q_pose, int flags, hipStream_t stream);

// sai2b_randomize_robots (sai2b_env_sampler.hip: env_randomize_kernel): the plant rows of the masked robots redrawn from their
// nominal rows in one launch. Its own parameter block, passed by value as a kernel argument; DevParams is not read. A pointer
// the groups of the call do not need may be NULL.
constexpr int ENV_COUNTS = 2;  // robots drawn, robots with a lag clipped at 1
struct EnvParams {
	unsigned groups = 0;  // bits of sai2b_env_group this call draws
	int both = 0;		  // the payload draw goes to the controller's rows too
	int* counter = nullptr;	 // [B]
	int* counts = nullptr;	 // [ENV_COUNTS], zeroed by the caller on the stream ahead of the launch
	double* sample = nullptr;  // [total][B]
	int sample_row[5] = {-1, -1, -1, -1, -1};  // first sample row of group g
	const double *nom_plant_payload = nullptr, *nom_payload = nullptr, *nom_contact = nullptr, *nom_joint = nullptr, *nom_actuator = nullptr,
				 *nom_sensor = nullptr;
	double *plant_payload = nullptr, *payload = nullptr, *contact = nullptr, *joint = nullptr, *actuator = nullptr, *sensor = nullptr,
		   *wrench = nullptr;
	HwStream rng;
	EnvDraw draw;
};
// mask [B] device bytes
int launch_env_randomize(int B, const EnvParams& p, const unsigned char* mask, hipStream_t stream);

// sai2b_collision_query (sai2b_collision.hip: collision_kernel): its own parameter block, passed by value as a kernel argument;
// DevParams is not read (the chain's constants are part of the law's block, sai2b_collision_law.h).
struct ColParams {
	ColLaw<N> law;
	const double* q = nullptr;	   // [N][B]: the truth, or the measured q (view)
	const double* rows = nullptr;  // [6 P + 4 O][B] or NULL without planes and obstacles
	double* out = nullptr;		   // [rows][B] or NULL
	unsigned char* flags = nullptr;	 // [B] or NULL
	int* counts = nullptr;		   // [COL_COUNTS], zeroed by the caller on the stream ahead of the launch
};
int launch_collision(int B, const ColParams& p, hipStream_t stream);
// sai2b_end_episodes (sai2b_collision.hip: end_episodes_kernel): the robots of `extra` that are not done yet are closed as step 5
// of observe_reward_kernel closes them, then done |= bit. state / episode: the reward's accumulators or NULL; steps: the
// observation's episode counters or NULL; count: one int, zeroed by the caller on the stream ahead of the launch
struct EndParams {
	unsigned char* done = nullptr;		   // [B]
	const unsigned char* extra = nullptr;  // [B]
	double* state = nullptr;			   // [REW_STATE_ROWS][B]
	int* episode = nullptr;				   // [REW_EPISODE_ROWS][B]
	int* steps = nullptr;				   // [B]
	int* count = nullptr;
	int bit = 0;
};
int launch_end_episodes(int B, const EndParams& p, hipStream_t stream);

// sai2b_solve_ik (sai2b_ik.hip: ik_kernel): its own parameter block, passed by value as a kernel argument; DevParams is not read
// (the chain, the task's frame and the clamped limits are part of the law's block, sai2b_ik_law.h).
struct IkParams {
	IkLaw<N> law;
	const double* goal = nullptr;		  // [12][B]: position 3, rotation 9 row-major (the call's rows or the task's goal rows)
	const double* rest = nullptr;		  // [N][B] or NULL (rest_weight == 0)
	const double* seed = nullptr;		  // [N][B]: the call's rows, or the state in the configured view
	const unsigned char* mask = nullptr;  // [B] or NULL: every robot
	double* q_out = nullptr;			  // [N][B]
	double* status = nullptr;			  // [IK_STATUS_ROWS][B]
	unsigned char* flags = nullptr;		  // [B]
	int* counts = nullptr;				  // [IK_COUNTS], zeroed by the caller on the stream ahead of the launch
};
int launch_ik(int B, const IkParams& p, hipStream_t stream);

}  // namespace sai2b

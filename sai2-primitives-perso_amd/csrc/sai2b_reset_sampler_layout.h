// sai2b_reset_sampler_layout.h — the per-robot rows of the episode sampler (include/sai2b.h "episode starts") and what the host
// checks of its configuration and of rows given as host arrays, decided from the configuration, the task list and the joint
// count alone. No HIP in here: sai2b_host.cpp uses it for the context, tests/cpp/reset_sampler_driver.cpp runs it on a CPU.
// (The functions are static: every per-size build has its own, and the library exports none of them.)
#pragma once
#include <cmath>
#include <cstddef>
#include <string>

#include "../../include/sai2b.h"

namespace sai2b {

// blocks of the rows, in storage order; the two goal blocks repeat per task of goal_tasks (MotionForceTasks first, in task
// order, then JointTasks)
enum RsBlock { RS_Q_LOWER = 0, RS_Q_UPPER, RS_DQ_SIGMA, RS_Q_NOMINAL, RS_GOAL_MFT, RS_GOAL_JT, RS_BLOCKS };
constexpr int RS_MFT_ROWS = 7;	// pos_lower 3, pos_upper 3, theta_max

struct RsLayout {
	int total = 0;
	int first[4] = {0, 0, 0, 0};					   // q_lower, q_upper, dq_sigma, q_nominal
	int goal_first[SAI2B_MAX_TASKS] = {-1, -1, -1, -1};  // first goal row of task t, -1: no goal is drawn for it
	int goal_rows[SAI2B_MAX_TASKS] = {0, 0, 0, 0};
};

// rows of a JointTask's goal block
static inline int rs_joint_rows(const sai2b_task_config& t, int dof) { return t.task_dof > 0 ? t.task_dof : dof; }

static inline RsLayout rs_layout(const sai2b_reset_sampler_config& c, const sai2b_task_config* tasks, int n_tasks, int dof) {
	RsLayout L;
	for (int k = 0; k < 4; k++) L.first[k] = k * dof;
	L.total = 4 * dof;
	for (int pass = 0; pass < 2; pass++)
		for (int t = 0; t < n_tasks && t < SAI2B_MAX_TASKS; t++) {
			if (!(c.goal_tasks >> t & 1u) || !tasks) continue;
			const bool mft = tasks[t].type == SAI2B_MOTION_FORCE_TASK;
			if (mft != (pass == 0)) continue;
			L.goal_first[t] = L.total;
			L.goal_rows[t] = mft ? RS_MFT_ROWS : rs_joint_rows(tasks[t], dof);
			L.total += L.goal_rows[t];
		}
	return L;
}

static inline bool rs_is_mft(const sai2b_task_config* tasks, int n_tasks, int t) {
	return tasks && t >= 0 && t < n_tasks && tasks[t].type == SAI2B_MOTION_FORCE_TASK;
}

// "" or the reason the configuration is rejected. has_contact: a contact is in force (use_clearance needs one)
static inline std::string rs_config_error(const sai2b_reset_sampler_config* c, const sai2b_task_config* tasks, int n_tasks, bool has_contact) {
	if (!c) return "reset sampler: null config";
	if (c->max_tries < 1 || c->max_tries > SAI2B_MAX_RESET_TRIES) return "reset sampler: max_tries must be in [1, SAI2B_MAX_RESET_TRIES]";
	if (n_tasks < 0 || n_tasks > SAI2B_MAX_TASKS || (n_tasks > 0 && !tasks)) return "reset sampler: bad task list";
	if (c->goal_tasks >> n_tasks) return "reset sampler: goal_tasks names a task the hierarchy does not have";
	for (int t = 0; t < n_tasks; t++)
		if ((c->absolute_position >> t & 1u) && !((c->goal_tasks >> t & 1u) && rs_is_mft(tasks, n_tasks, t)))
			return "reset sampler: absolute_position names a task that is not a MotionForceTask of goal_tasks";
	if (c->absolute_position >> n_tasks) return "reset sampler: absolute_position names a task that is not a MotionForceTask of goal_tasks";
	if (c->ratio_task != -1 && !rs_is_mft(tasks, n_tasks, c->ratio_task)) return "reset sampler: ratio_task must be -1 or the index of a MotionForceTask";
	if (c->ratio_task != -1 && !(c->min_ratio >= 0 && c->min_ratio <= 1)) return "reset sampler: min_ratio must be in [0, 1]";
	if (c->box_task != -1 && !rs_is_mft(tasks, n_tasks, c->box_task)) return "reset sampler: box_task must be -1 or the index of a MotionForceTask";
	if (c->box_task != -1)
		for (int k = 0; k < 3; k++)
			if (!std::isfinite(c->box_lower[k]) || !std::isfinite(c->box_upper[k])) return "reset sampler: the box must be finite";
	if (c->use_clearance != 0 && c->use_clearance != 1) return "reset sampler: use_clearance must be 0 or 1";
	if (c->use_clearance && !std::isfinite(c->clearance)) return "reset sampler: clearance must be finite";
	if (c->use_clearance && !has_contact) return "reset sampler: use_clearance needs a contact (sai2b_set_contact)";
	return "";
}

// "" or the reason host rows [total][B] are rejected; model limits q_min / q_max [dof]
static inline std::string rs_rows_error(const RsLayout& L, const sai2b_task_config* tasks, int n_tasks, int dof, const double* q_min,
										const double* q_max, const double* rows, size_t B) {
	const double pi = 3.141592653589793;
	for (size_t i = 0; i < (size_t)L.total * B; i++)
		if (!std::isfinite(rows[i])) return "reset sampler: every row must be finite";
	for (int i = 0; i < dof; i++)
		for (size_t b = 0; b < B; b++) {
			const double lo = rows[(size_t)(L.first[RS_Q_LOWER] + i) * B + b], hi = rows[(size_t)(L.first[RS_Q_UPPER] + i) * B + b];
			const double sg = rows[(size_t)(L.first[RS_DQ_SIGMA] + i) * B + b], nom = rows[(size_t)(L.first[RS_Q_NOMINAL] + i) * B + b];
			if (!(lo <= hi)) return "reset sampler: q_lower must not exceed q_upper";
			if (sg < 0) return "reset sampler: dq_sigma must not be negative";
			if (!(nom >= q_min[i] && nom <= q_max[i])) return "reset sampler: q_nominal must lie within the model's joint limits";
		}
	for (int t = 0; t < n_tasks; t++) {
		if (L.goal_first[t] < 0) continue;
		if (tasks[t].type == SAI2B_MOTION_FORCE_TASK) {
			for (size_t b = 0; b < B; b++) {
				const double th = rows[(size_t)(L.goal_first[t] + 6) * B + b];
				if (!(th >= 0 && th <= pi)) return "reset sampler: theta_max must be in [0, pi]";
			}
		} else {
			for (size_t i = 0; i < (size_t)L.goal_rows[t] * B; i++)
				if (rows[(size_t)L.goal_first[t] * B + i] < 0) return "reset sampler: half_width must not be negative";
		}
	}
	return "";
}

// the default rows: the middle 80 % of the joint range, no velocity, the middle of the range as the nominal posture, goals at
// the start pose
static inline void rs_default_rows(const RsLayout& L, int dof, const double* q_min, const double* q_max, size_t B, double* rows) {
	for (size_t i = 0; i < (size_t)L.total * B; i++) rows[i] = 0.0;
	for (int i = 0; i < dof; i++) {
		const double mid = 0.5 * (q_min[i] + q_max[i]), half = 0.5 * (q_max[i] - q_min[i]);
		for (size_t b = 0; b < B; b++) {
			rows[(size_t)(L.first[RS_Q_LOWER] + i) * B + b] = mid - 0.8 * half;
			rows[(size_t)(L.first[RS_Q_UPPER] + i) * B + b] = mid + 0.8 * half;
			rows[(size_t)(L.first[RS_Q_NOMINAL] + i) * B + b] = mid;
		}
	}
}

}  // namespace sai2b

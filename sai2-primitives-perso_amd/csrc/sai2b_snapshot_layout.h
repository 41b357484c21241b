// sai2b_snapshot_layout.h — what a snapshot bank holds per robot, decided on the host from a description of the context alone:
// the joint count, every task's kind, size, generator mode and observer, and which optional buffers exist. No HIP in here:
// sai2b_host.cpp describes its context, uploads the table with each block's base pointer and the kernels of
// sai2b_snapshot.hip read only that; tests/cpp/snapshot_layout_driver.cpp runs the same code on a CPU.
// (The functions are static: every per-size build has its own, and the library exports none of them.)
#pragma once
#include <cstdio>
#include <cstring>

#include "sai2b_params.h"

namespace sai2b {

// the blocks of a robot's state, in the order of their ids. "Episode" blocks are what sai2b_reset_robots replaces or what advances
// with time, "environment" blocks are what it documents as kept.
enum SnapBlock {
	// ---- SAI2B_SNAP_EPISODE
	SNAP_Q = 0, SNAP_DQ, SNAP_TAU, SNAP_Q_POSE,	 // [dof] rows each
	SNAP_GOALS, SNAP_SENSED, SNAP_STATE, SNAP_ISTATE, SNAP_OTG_DESIRED, SNAP_OTG_STATE, SNAP_OTG3_TRAJ, SNAP_POPC_F, SNAP_POPC_I, SNAP_POPC_Q,
	SNAP_NPREC,				// per task
	SNAP_EPISODE_STEP,		// the observation's per-robot step counter (int)
	SNAP_WRENCH_REMAINING,	// the remaining-periods row of the external wrench
	SNAP_CONTACT_STATUS, SNAP_JOINT_STATUS, SNAP_WRENCH_STATUS,
	// ---- SAI2B_SNAP_ENVIRONMENT
	SNAP_PAYLOAD, SNAP_PLANT_PAYLOAD, SNAP_CONTACT, SNAP_JOINT, SNAP_WRENCH,
	// ---- appended for the actuator and sensor models (sai2b_set_hardware): ids stay what exported blobs hold. Episode: the torque
	// history, the filter states f and g, the applied torques, the clocks (period, episode; int); environment: the two row buffers.
	// In a description they stand with their group: snap_block_order()
	SNAP_HW_HISTORY, SNAP_HW_FILTER, SNAP_HW_APPLIED, SNAP_HW_CLOCK, SNAP_HW_ACTUATOR, SNAP_HW_SENSOR,
	// ---- appended for the reward's accumulators (sai2b_set_reward), both episode: return, discount, last return, tau_prev; last
	// length and tau_prev's valid flag (int)
	SNAP_REWARD_STATE, SNAP_REWARD_EPISODE,
	// ---- appended for the episode sampler (sai2b_set_reset_sampler), episode: the per-robot episode counter its draws are keyed by (int)
	SNAP_RS_EPISODE,
	SNAP_BLOCKS,  // the blocks up to the episode sampler's (a test pins the value)
	// ---- appended for the environment sampler (sai2b_set_env_sampler): its per-robot draw counter (int), episode; the drawn
	// quantities (the sample rows), environment: they travel with the plant rows they describe
	SNAP_ES_COUNTER = SNAP_BLOCKS, SNAP_ES_SAMPLE,
	SNAP_BLOCKS_ALL,  // the blocks up to the environment sampler's (a test pins this value too)
	// ---- appended for the joint sensors (sai2b_set_joint_sensor). Episode: the measured q and dq, the previous position reading,
	// the velocity filter's state, the history of readings, the clock (next reading, episode; int); environment: the rows
	SNAP_JS_Q = SNAP_BLOCKS_ALL, SNAP_JS_DQ, SNAP_JS_PREV, SNAP_JS_FILTER, SNAP_JS_HISTORY, SNAP_JS_CLOCK, SNAP_JS_ROWS,
	SNAP_BLOCKS_EVERY
};
static const char* const SNAP_BLOCK_NAME[SNAP_BLOCKS_EVERY] = {
	"q", "dq", "tau", "q_pose", "goals", "sensed", "state", "istate", "otg_desired", "otg_state", "otg3_traj", "popc_f", "popc_i", "popc_q",
	"N_prec", "episode_step", "wrench_remaining", "contact_status", "joint_status", "wrench_status",
	"payload", "plant_payload", "contact", "joint_dynamics", "external_wrench",
	"hw_history", "hw_filter", "hw_applied", "hw_clock", "hw_actuator", "hw_sensor", "reward_state", "reward_episode",
	"reset_sampler_episode", "env_sampler_counter", "env_sampler_sample",
	"joint_sensor_q", "joint_sensor_dq", "joint_sensor_previous", "joint_sensor_filter", "joint_sensor_history", "joint_sensor_clock",
	"joint_sensor_rows"};
// where a block stands in the sequence snapshot_blocks() draws from: the hardware's, the reward's and the two samplers' episode
// blocks ahead of the environment group, the environment sampler's sample rows at its end; the joint sensors' episode blocks
// behind the episode group's last, their rows behind the environment group's last
static inline int snap_block_order_base(int block);
static inline int snap_block_order(int block) {	 // eight places behind every earlier block, for those appended since
	if (block >= SNAP_JS_Q && block <= SNAP_JS_CLOCK) return 8 * snap_block_order_base(SNAP_ES_COUNTER) + 1 + (block - SNAP_JS_Q);
	if (block == SNAP_JS_ROWS) return 8 * snap_block_order_base(SNAP_ES_SAMPLE) + 1;
	return 8 * snap_block_order_base(block);
}
static inline int snap_block_order_base(int block) {
	constexpr int hw_episode = SNAP_HW_CLOCK - SNAP_HW_HISTORY + 1, reward = SNAP_REWARD_EPISODE - SNAP_REWARD_STATE + 1;
	constexpr int environment = SNAP_WRENCH - SNAP_PAYLOAD + 1, hw_environment = SNAP_HW_SENSOR - SNAP_HW_ACTUATOR + 1, sampler = 2;
	if (block >= SNAP_PAYLOAD && block <= SNAP_WRENCH) return block + hw_episode + reward + sampler;
	if (block >= SNAP_HW_HISTORY && block <= SNAP_HW_CLOCK) return block - environment;
	if (block >= SNAP_REWARD_STATE && block <= SNAP_REWARD_EPISODE) return block - environment - hw_environment;
	if (block == SNAP_RS_EPISODE || block == SNAP_ES_COUNTER) return block - environment - hw_environment;
	if (block >= SNAP_HW_ACTUATOR && block <= SNAP_HW_SENSOR) return block + reward + sampler;
	return block;
}

constexpr int SNAP_EPISODE_BIT = 1, SNAP_ENVIRONMENT_BIT = 2;  // SAI2B_SNAP_EPISODE, SAI2B_SNAP_ENVIRONMENT
// rows of the plant's optional buffers (sai2b_launch.h has the same numbers for the kernels; sai2b_host.cpp asserts they agree)
constexpr int SNAP_JOINT_ROWS = 6, SNAP_JOINT_STATUS_ROWS = 3, SNAP_WRENCH_MOTION_ROWS = 6, SNAP_POPC_F_ROWS = 4, SNAP_POPC_I_ROWS = 3;
constexpr int SNAP_HW_SENSOR_ROWS = 13, SNAP_HW_MAX_DEPTH = 8;

// one task as the layout sees it
struct SnapTaskDesc {
	int kind;	   // SAI2B_JOINT_TASK / SAI2B_MOTION_FORCE_TASK
	int k0;		   // rows of a JointTask (0 for a MotionForceTask)
	int otg_mode;  // 0 = generator off, 1 = acceleration-limited, 2 = jerk-limited
	int otg3;	   // the jerk-limited generator's trajectory buffer exists
	int popc;	   // the passivity observer's buffers exist
	int nprec;	   // the task-level N_prec buffer exists
};
// the context as the layout sees it; fields the chosen groups do not read are zero (sai2b_host.cpp: snapshot_describe)
struct SnapDesc {
	int dof, n_tasks, what;
	SnapTaskDesc task[SAI2B_MAX_TASKS];
	int steps;						 // observation step counters exist
	int contact, joint, wrench;		 // the plant's optional buffers exist
	int payload, plant_payload;
	int hardware;		 // the buffers of the actuator and sensor models exist (0: none, and hardware_depth is 0)
	int hardware_depth;	 // D: the torque history holds D + 1 periods
	int reward;			 // the reward's accumulators exist
	int reset_sampler;	 // the episode sampler's counter exists
	int env_sampler;	 // 0: no environment sampler; else 1 + its sample rows
	int joint_sensor;	 // the joint sensors' buffers exist (0: none, and joint_sensor_depth is 0)
	int joint_sensor_depth;	 // D: the history of readings holds D + 1 periods. Appended: code that zeroes a description and fills
							 // the fields above stays valid
};

struct SnapRow {
	int block, task;  // SnapBlock; task index or -1
	int rows;		  // [rows][B] elements in the context
	int elem_bytes;	  // 4 (int) or 8 (double)
	int first_word;	  // first 4-byte word of the block in a robot's bank column
	int first_row;	  // rows of all blocks before this one
};
constexpr int SNAP_MAX_ROWS_TABLE = 9 + 11 * SAI2B_MAX_TASKS + 5 + 6 + 2;	 // the blocks up to the reward's (a description without the sampler)
constexpr int SNAP_TABLE_CAPACITY = SNAP_MAX_ROWS_TABLE + 1;			 // and the episode sampler's (a test pins this value too)
constexpr int SNAP_TABLE_ROOM = SNAP_TABLE_CAPACITY + 2;				 // and the environment sampler's two (a test pins this value too)
constexpr int SNAP_TABLE_FULL = SNAP_TABLE_ROOM + 7;					 // and the joint sensors' seven: what every table below has room for

struct SnapLayout {
	int n = 0;
	int words = 0, rows = 0;  // per robot
	unsigned long long fingerprint = 0;
	SnapRow row[SNAP_TABLE_FULL];
};

static inline int snap_goal_rows(const SnapTaskDesc& t) { return t.kind == SAI2B_MOTION_FORCE_TASK ? MFT_GOAL_ROWS : 3 * t.k0; }

// the blocks of a description in id order, without their words: (block, task, rows, element bytes)
static inline int snapshot_blocks(const SnapDesc& d, SnapRow* out) {
	int n = 0;
	auto add = [&](int block, int task, int rows, int bytes) {
		if (rows > 0) out[n++] = SnapRow{block, task, rows, bytes, 0, 0};
	};
	if (d.what & SNAP_EPISODE_BIT) {
		for (int blk = SNAP_Q; blk <= SNAP_Q_POSE; blk++) add(blk, -1, d.dof, 8);
		for (int t = 0; t < d.n_tasks; t++) {
			const SnapTaskDesc& k = d.task[t];
			const bool mft = k.kind == SAI2B_MOTION_FORCE_TASK;
			add(SNAP_GOALS, t, snap_goal_rows(k), 8);
			add(SNAP_SENSED, t, mft ? 6 : 0, 8);
			add(SNAP_STATE, t, mft ? 12 + 3 * d.dof : k.k0, 8);
			add(SNAP_ISTATE, t, mft ? MFT_ISTATE_ROWS : 0, 4);
			add(SNAP_OTG_DESIRED, t, snap_goal_rows(k), 8);
			add(SNAP_OTG_STATE, t, OTG_ROWS, 8);
			add(SNAP_OTG3_TRAJ, t, k.otg3 ? OTG_MD * OTG3_STRIDE : 0, 8);
			add(SNAP_POPC_F, t, k.popc ? SNAP_POPC_F_ROWS : 0, 8);
			add(SNAP_POPC_I, t, k.popc ? SNAP_POPC_I_ROWS : 0, 4);
			add(SNAP_POPC_Q, t, k.popc ? POPC_RING : 0, 8);
			add(SNAP_NPREC, t, k.nprec ? d.dof * d.dof : 0, 8);
		}
		add(SNAP_EPISODE_STEP, -1, d.steps ? 1 : 0, 4);
		add(SNAP_WRENCH_REMAINING, -1, d.wrench ? 1 : 0, 8);
		add(SNAP_CONTACT_STATUS, -1, d.contact ? CONTACT_STATUS_ROWS : 0, 8);
		add(SNAP_JOINT_STATUS, -1, d.joint ? SNAP_JOINT_STATUS_ROWS * d.dof : 0, 8);
		add(SNAP_WRENCH_STATUS, -1, d.wrench ? 6 + d.dof : 0, 8);
		add(SNAP_HW_HISTORY, -1, d.hardware ? (d.hardware_depth + 1) * d.dof : 0, 8);
		add(SNAP_HW_FILTER, -1, d.hardware ? d.dof + 6 : 0, 8);
		add(SNAP_HW_APPLIED, -1, d.hardware ? d.dof : 0, 8);
		add(SNAP_HW_CLOCK, -1, d.hardware ? 2 : 0, 4);
		add(SNAP_REWARD_STATE, -1, d.reward ? 3 + d.dof : 0, 8);
		add(SNAP_REWARD_EPISODE, -1, d.reward ? 2 : 0, 4);
		add(SNAP_RS_EPISODE, -1, d.reset_sampler ? 1 : 0, 4);
		add(SNAP_ES_COUNTER, -1, d.env_sampler ? 1 : 0, 4);
		for (int blk = SNAP_JS_Q; blk <= SNAP_JS_FILTER; blk++) add(blk, -1, d.joint_sensor ? d.dof : 0, 8);
		add(SNAP_JS_HISTORY, -1, d.joint_sensor ? (d.joint_sensor_depth + 1) * 2 * d.dof : 0, 8);
		add(SNAP_JS_CLOCK, -1, d.joint_sensor ? 2 : 0, 4);
	}
	if (d.what & SNAP_ENVIRONMENT_BIT) {
		add(SNAP_PAYLOAD, -1, d.payload ? PAYLOAD_ROWS : 0, 8);
		add(SNAP_PLANT_PAYLOAD, -1, d.plant_payload ? PAYLOAD_ROWS : 0, 8);
		add(SNAP_CONTACT, -1, d.contact ? CONTACT_ROWS : 0, 8);
		add(SNAP_JOINT, -1, d.joint ? SNAP_JOINT_ROWS * d.dof : 0, 8);
		add(SNAP_WRENCH, -1, d.wrench ? SNAP_WRENCH_MOTION_ROWS : 0, 8);
		add(SNAP_HW_ACTUATOR, -1, d.hardware ? 1 + 3 * d.dof : 0, 8);
		add(SNAP_HW_SENSOR, -1, d.hardware ? SNAP_HW_SENSOR_ROWS : 0, 8);
		add(SNAP_ES_SAMPLE, -1, d.env_sampler ? d.env_sampler - 1 : 0, 8);
		add(SNAP_JS_ROWS, -1, d.joint_sensor ? 1 + 5 * d.dof : 0, 8);
	}
	return n;
}

// FNV-1a over the integers of a description (field by field: no padding is hashed)
static inline unsigned long long snapshot_fingerprint(const SnapDesc& d) {
	unsigned long long h = 1469598103934665603ull;
	auto mix = [&](int v) {
		for (int i = 0; i < 4; i++) h = (h ^ (unsigned long long)(((unsigned)v >> (8 * i)) & 0xffu)) * 1099511628211ull;
	};
	mix(d.dof), mix(d.n_tasks), mix(d.what);
	for (int t = 0; t < SAI2B_MAX_TASKS; t++) {
		const SnapTaskDesc& k = d.task[t];
		mix(k.kind), mix(k.k0), mix(k.otg_mode), mix(k.otg3), mix(k.popc), mix(k.nprec);
	}
	mix(d.steps), mix(d.contact), mix(d.joint), mix(d.wrench), mix(d.payload), mix(d.plant_payload);
	// only with the feature: a description without it keeps the fingerprint it had before the fields existed
	if (d.hardware != 0) mix(d.hardware), mix(d.hardware_depth);
	if (d.reward != 0) mix(d.reward);
	if (d.reset_sampler != 0) mix(d.reset_sampler);
	if (d.env_sampler != 0) mix(d.env_sampler);
	if (d.joint_sensor != 0) mix(d.joint_sensor), mix(d.joint_sensor_depth);
	return h;
}

// The row table: the 8-byte blocks first, then the 4-byte ones, each in id order, so that an 8-byte block starts at an even word
// and stays 8-byte aligned in a [word][capacity] bank of any capacity. Words are contiguous.
static inline SnapLayout snapshot_layout(const SnapDesc& d) {
	SnapLayout L;
	SnapRow all[SNAP_TABLE_FULL];
	const int n = snapshot_blocks(d, all);
	for (int bytes = 8; bytes >= 4; bytes -= 4)
		for (int i = 0; i < n; i++) {
			if (all[i].elem_bytes != bytes) continue;
			SnapRow r = all[i];
			r.first_word = L.words, r.first_row = L.rows;
			L.words += r.rows * (bytes / 4), L.rows += r.rows;
			L.row[L.n++] = r;
		}
	L.fingerprint = snapshot_fingerprint(d);
	return L;
}

// the first block in which two descriptions differ, as text for an error message; false: they are equal
static inline bool snapshot_first_difference(const SnapDesc& a, const SnapDesc& b, char* msg, int len) {
	if (a.dof != b.dof) return std::snprintf(msg, len, "block q: %d joints against %d", a.dof, b.dof), true;
	if (a.what != b.what) return std::snprintf(msg, len, "block q: groups %d against %d", a.what, b.what), true;
	SnapRow ra[SNAP_TABLE_FULL], rb[SNAP_TABLE_FULL];
	const int na = snapshot_blocks(a, ra), nb = snapshot_blocks(b, rb);
	for (int i = 0; i < (na < nb ? na : nb); i++) {
		const SnapRow &x = ra[i], &y = rb[i];
		if (x.block == y.block && x.task == y.task && x.rows == y.rows) {
			// the generator mode does not change the rows, but it changes what they mean
			if (x.block == SNAP_OTG_STATE && a.task[x.task].otg_mode != b.task[x.task].otg_mode)
				return std::snprintf(msg, len, "block otg_state of task %d: generator mode %d against %d", x.task, a.task[x.task].otg_mode,
									 b.task[x.task].otg_mode), true;
			continue;
		}
		// both lists are drawn from one sequence (globals, then task by task, then the optional features): the earlier entry is missing in the other
		auto key = [](const SnapRow& r) {
			const int grp = r.block < SNAP_GOALS ? 0 : r.block <= SNAP_NPREC ? 1 : 2;
			return (grp * 16 + (r.task < 0 ? 0 : r.task)) * 512 + snap_block_order(r.block);
		};
		const SnapRow& first = key(x) <= key(y) ? x : y;
		if (first.task >= 0) return std::snprintf(msg, len, "block %s of task %d", SNAP_BLOCK_NAME[first.block], first.task), true;
		return std::snprintf(msg, len, "block %s", SNAP_BLOCK_NAME[first.block]), true;
	}
	if (na != nb) {
		const SnapRow& r = na > nb ? ra[nb] : rb[na];
		if (r.task >= 0) return std::snprintf(msg, len, "block %s of task %d", SNAP_BLOCK_NAME[r.block], r.task), true;
		return std::snprintf(msg, len, "block %s", SNAP_BLOCK_NAME[r.block]), true;
	}
	if (std::memcmp(&a, &b, sizeof(SnapDesc)) != 0 || snapshot_fingerprint(a) != snapshot_fingerprint(b))
		return std::snprintf(msg, len, "block q: the descriptions differ in a field without rows"), true;
	return false;
}

}  // namespace sai2b

// sai2b_tick_policy.h — what a tick launches, decided on the host from host data alone: the hierarchy, the switches of the
// environment and three integers that come back from the device every eighth tick. No HIP in here: sai2b_host.cpp asks,
// fetches the counts and issues what plan() names; tests/cpp/tick_policy_driver.cpp runs the same code on a CPU.
// (The functions are static: every per-size build has its own, and the library exports none of them.)
#pragma once
#include <algorithm>
#include <cstdlib>

#include "sai2b_params.h"

namespace sai2b {

// which first kernel a tick runs
struct TickForm {
	int fast = 0;  // 0 = the generic kernel alone, 1 = [full MFT], 2 = [full MFT, full JT], 3 + rows = tick_cert_kernel
				   // (rows: most rows of a partial task of the hierarchy)
	bool baked = false;			  // robot constants from the compile-time Panda (tick_fast_kernel)
	bool payload = false;		  // the context has per-robot payloads: the SVD-free kernels' payload forms (the generic
								  // kernels find the rows in the parameter block)
	bool inlane_singular = true;  // singular MotionForceTasks stay in the lane (cert::singular_part), not on the work list
	bool sing6 = false;			  // the 6-row tick_cert_kernel with the singular branch in the lane (cert::tick<.., S6>)
	bool self = false;			  // fast = 1 | 2 without payload: one launch, each wavefront serves the robots it declines itself
								  // (tick_self_kernel, sai2b_self.hip) instead of the generic kernel over a work list behind
};

// what a tick call asks for
struct TickCall {
	bool debug = false;	 // the introspection instantiation of the generic kernel, no SVD-free kernel
	bool commit_sh = true, with_comp = true, do_torque = true;
	int group = 0;	// lanes per robot of the generic kernel (16 / 8), or 0 = the one-lane-per-robot generic kernel
	unsigned stamp = 0;	 // != 0: the host asks for the work list's counts, tagged with it (WorkList::report)
};

// ------------------------------------------------------------------------------------------------
// thresholds
// ------------------------------------------------------------------------------------------------
// A count recorded at tick k is consumed at the first tick >= k + LOOK_DISTANCE, waiting for the read-back if it has not
// arrived (it has, at that distance, unless the caller never fetches a result); the next one is recorded there.
constexpr int LOOK_DISTANCE = 8;
// The numbers of the singular mode and the back-off are the measured break-even on the Panda (scripts/micro/sing6_crossover.py:
// 65 536 robots, 14 890 declined: 173 us against 215 us with the 6-row kernel; 22 382 declined: 238 against 195): the in-lane
// 6-row branch costs every wavefront ~100 us whatever the batch, a pass over the work list ~60 us per round of 4 096 robots
// (16 lanes each) or ~450 us per 65 536 in its throughput form.
constexpr int SING6_ENTER = 20480;	// more robots than this leave the hierarchy's own kernel for the work list: the 6-row kernel
constexpr int SING6_LEAVE = 15360;	// fewer than this either take its in-lane branch or leave it: back to the hierarchy's own
// a kernel for general hierarchies that keeps less than 60 % of the batch (declined * DEN > B * NUM) rests for BACKOFF_TICKS
constexpr int BACKOFF_NUM = 2, BACKOFF_DEN = 5, BACKOFF_TICKS = 64;
// what the pass over a work list serves in one round with 16 lanes per robot: 4 robots x 1024 wavefronts. A longer list is
// throughput, not latency (two robots per DPP row, as for a whole batch), and too long for the one-launch form
constexpr int PASS_ROUND = 4096;
// one round of the self form's tail: the four 16-lane groups of a wavefront take one declined robot each
constexpr int SELF_WAVE_ROUND = 4;
// a whole batch of at least this many robots fills the machine with 8 lanes per robot
constexpr int BATCH_8_LANES = 16384;
// sai2b_cert.hpp: deferred stores per robot (PEND_SLOTS), and the rows of a partial task the kernel is instantiated for
constexpr int CERT_PEND_SLOTS = 36, CERT_MAX_ROWS = 6;
// tick_cert_kernel<6, S6> serves the blending regions of MotionForceTasks of at least this many rows
constexpr int SING6_MIN_ROWS = 4;

// ------------------------------------------------------------------------------------------------
// switches of the environment (read once, when a context is created)
// ------------------------------------------------------------------------------------------------
static inline bool env_flag(const char* name) {
	const char* v = std::getenv(name);
	return v && v[0] == '1';
}

struct RouteSwitches {
	bool no_fast_path = false;		  // SAI2B_NO_FAST_PATH=1: always run the generic kernel
	bool no_cert_path = false;		  // SAI2B_NO_CERT_PATH=1: no SVD-free kernel for general hierarchies (sai2b_cert.hpp)
	bool no_task_cert = false;		  // SAI2B_NO_TASK_CERT=1: the generic task_kernel for every robot (A/B)
	bool no_inlane_singular = false;  // SAI2B_NO_INLANE_SINGULAR=1: singular MotionForceTasks of tick_cert_kernel<3> go to the work list
	bool no_sing6 = false;			  // SAI2B_NO_SING6=1: never the 6-row kernel with the singular branch in the lane
	bool force_sing6 = false;		  // SAI2B_FORCE_SING6=1 (testing aid): that kernel from the first tick on, whatever the counts
	bool prefer_cert = false;		  // SAI2B_PREFER_CERT=1 (diagnostic): sai2b_cert.hpp also where sai2b_fast.hpp applies
	bool no_self_serve = false;		  // SAI2B_NO_SELF_SERVE=1: the headline tick keeps its two launches
	// lanes per robot of the generic kernel: SAI2B_GENERIC_LANES = 16 / 8 / 1 (1: the one-lane-per-robot kernel),
	// default 0 = by the amount of work (generic_lanes())
	int generic_lanes_env = 0;
};

static inline RouteSwitches route_switches_from_env() {
	RouteSwitches sw;
	sw.no_fast_path = env_flag("SAI2B_NO_FAST_PATH");
	sw.no_cert_path = env_flag("SAI2B_NO_CERT_PATH");
	sw.no_task_cert = env_flag("SAI2B_NO_TASK_CERT");
	sw.no_inlane_singular = env_flag("SAI2B_NO_INLANE_SINGULAR");
	sw.no_sing6 = env_flag("SAI2B_NO_SING6");
	sw.force_sing6 = env_flag("SAI2B_FORCE_SING6");
	sw.prefer_cert = env_flag("SAI2B_PREFER_CERT");
	sw.no_self_serve = env_flag("SAI2B_NO_SELF_SERVE");
	if (const char* gl = std::getenv("SAI2B_GENERIC_LANES")) sw.generic_lanes_env = std::atoi(gl);
	return sw;
}

// ------------------------------------------------------------------------------------------------
// which kernels a hierarchy is eligible for
// ------------------------------------------------------------------------------------------------
// the hierarchy as the policy reads it: the flattened tasks of the parameter block, the configurations they came from, the
// model's joint types ([N], enum sai2b_joint_type)
struct Hierarchy {
	const DevParams* params = nullptr;
	const sai2b_task_config* cfg = nullptr;
	int T = 0;
	const int* joint_type = nullptr;
};

// 3 + r: the SVD-free kernel for general hierarchies (sai2b_cert.hpp): any robot size and joint type, any sequence
// of tasks whose rows can all be independent (at most N of them, a full JointTask only at the bottom); r = most
// rows a partial task brings (selects the kernel's instantiation); 0: not eligible
static inline int cert_kind(const RouteSwitches& sw, const Hierarchy& h) {
	if (sw.no_fast_path || sw.no_cert_path || h.T < 1) return 0;
	int rows = 0, max_rows = 0, slots = N;
	for (int t = 0; t < h.T; t++) {
		const DevTask& d = h.params->task[t];
		if (d.type == SAI2B_MOTION_FORCE_TASK) {
			// the passivity observer mutates per-robot state inside the law: generic kernel only
			if (h.cfg[t].passivity_enabled && h.cfg[t].closed_loop_force) return 0;
			rows += d.rank;
			max_rows = std::max(max_rows, d.rank);
			slots += 12;
		} else {
			if (d.full_selection && t != h.T - 1) return 0;
			rows += d.full_selection ? 0 : d.k0;
			if (!d.full_selection) max_rows = std::max(max_rows, d.k0);
			slots += d.k0;
		}
	}
	return (rows <= N && slots <= CERT_PEND_SLOTS && max_rows <= CERT_MAX_ROWS) ? 3 + max_rows : 0;
}

// eligibility of the SVD-free path (sai2b_fast.hpp): 1 = [full MFT], 2 = [full MFT, full JT] (any batch size: a robot
// the kernel declines goes to the generic kernel on its own, lanes past the batch just exit); else `cert`, the
// hierarchy's cert_kind()
static inline int fast_kind(const RouteSwitches& sw, const Hierarchy& h, int cert) {
	// these two kernels are written for 7 revolute joints (a 6-DOF task leaves a one-dimensional nullspace)
	bool arm7 = N == 7;
	for (int i = 0; i < N; i++)
		if (h.joint_type[i] != SAI2B_REVOLUTE) arm7 = false;
	if (!arm7 || sw.no_fast_path || h.T > 2 || h.cfg[0].type != SAI2B_MOTION_FORCE_TASK || !h.params->task[0].full_projection ||
		h.params->task[0].rank != 6 || (h.cfg[0].passivity_enabled && h.cfg[0].closed_loop_force))
		return cert;
	if (sw.prefer_cert && cert) return cert;
	if (h.T == 1) return 1;
	return (h.cfg[1].type == SAI2B_JOINT_TASK && h.params->task[1].full_selection) ? 2 : cert;
}

// The kernel for batches with many robots inside a blending region of a 4- to 6-row MotionForceTask: tick_cert_kernel<6, S6>
// (cert::singular_streamed); 0 when the hierarchy has no such task or is not the SVD-free kernel's
static inline int sing6_kind(const RouteSwitches& sw, int cert) {
	if (sw.no_inlane_singular || sw.no_sing6) return 0;
	return cert >= 3 + SING6_MIN_ROWS ? cert : 0;
}

// the three, computed once per call and passed on
struct RouteKinds {
	int cert = 0, fast = 0, sing6 = 0;
};
static inline RouteKinds route_kinds(const RouteSwitches& sw, const Hierarchy& h) {
	RouteKinds k;
	k.cert = cert_kind(sw, h);
	k.fast = fast_kind(sw, h, k.cert);
	k.sing6 = sing6_kind(sw, k.cert);
	return k;
}

// Rows of a task when the SVD-free task-level kernel (sai2b_cert.hip: task_cert_kernel) can serve it, else 0: the
// eligibility of cert_kind() for this one task. Not with introspection (its outputs come from the generic kernel) nor
// a passivity observer (it mutates state inside the law).
static inline int task_cert_rows(const RouteSwitches& sw, const Hierarchy& h, int task, bool introspection) {
	if (sw.no_task_cert || sw.no_fast_path || sw.no_cert_path || introspection) return 0;
	const DevTask& d = h.params->task[task];
	if (d.type == SAI2B_MOTION_FORCE_TASK) {
		if (h.cfg[task].passivity_enabled && h.cfg[task].closed_loop_force) return 0;
		return (d.rank >= 1 && d.rank <= CERT_MAX_ROWS) ? d.rank : 0;
	}
	if (d.full_selection) return 1;	 // (a full JointTask brings no level of its own: the small instantiation)
	return d.k0 <= CERT_MAX_ROWS ? d.k0 : 0;
}

// How many lanes a robot gets in the generic kernel (sai2b_group.hip). 16 = one DPP row per robot: the shortest
// critical path, what the (usually short) work list behind the SVD-free kernel wants; 8 = two robots per row:
// fewer idle lanes, better when the whole batch runs the generic kernel and fills the machine anyway.
// 0 = the one-lane-per-robot kernel.
static inline int generic_lanes(const RouteSwitches& sw, int B, bool whole_batch) {
	if (sw.generic_lanes_env == 1) return 0;
	if (sw.generic_lanes_env == 8 || sw.generic_lanes_env == 16) return sw.generic_lanes_env;
	return (whole_batch && B >= BATCH_8_LANES) ? 8 : 16;
}

// ------------------------------------------------------------------------------------------------
// the route of a tick and its state
// ------------------------------------------------------------------------------------------------
// something the device was asked for at tick k and the host consumes at the first tick >= k + LOOK_DISTANCE, one request
// at a time (the work list's counts; the generators' busy count)
struct DelayedLook {
	long long tick = 0, asked_at = 0;
	bool pending = false;
	// a tick begins; true: the pending request is due, and taken (also when the answer then never arrives: the next
	// tick asks afresh)
	bool advance() {
		tick++;
		if (!pending || tick - asked_at < LOOK_DISTANCE) return false;
		pending = false;
		return true;
	}
	void ask() { pending = true, asked_at = tick; }
};

// How many robots the SVD-free kernel for general hierarchies keeps is a property of the workload (a 6-DOF task
// behind a partial JointTask is inside a blending region most of the time), so the route of a tick is a function of
// the tick index, counted in ticks that want the SVD-free kernel, and of what the looks said.
struct TickRoute {
	// many robots inside a blending region of a 4- to 6-row MotionForceTask: the 6-row SVD-free kernel with the singular branch
	// in the lane runs instead of the hierarchy's usual first kernel
	bool sing_mode = false;
	int backoff = 0;	   // ticks left that run the generic kernel alone, then the SVD-free kernel is tried again
	DelayedLook look;	   // the work list's counts
	unsigned stamp = 0;	   // tag of the last request that went through the mapped words (never 0)
	bool by_copy = false;  // the pending request went through the two copies and the event instead
	int last_seen = -1;	   // length of the work list when the host last looked (-1: never)
	int last_wmax = -1;	   // most robots one wavefront declined, at that look (-1: not known, the look went through the copies)
	int last_form = 0;	   // the last tick: 0 = the generic kernel alone, 1 = two launches, 2 = the self form
	bool last_generic_only = false;	 // the last call was a plain torque tick that ran the generic kernel for every robot

	explicit TickRoute(const RouteSwitches& sw = RouteSwitches()) : sing_mode(sw.force_sing6) {}
	int pending() const { return look.pending ? (by_copy ? 2 : 1) : 0; }  // 1: by the mapped words, 2: by copies
};

// what the caller of a tick asks for, and what the context holds
struct TickAsk {
	bool introspection = false;
	int commit_sh = 1, with_comp = 1, do_torque = 1;
	bool payload = false;  // the context has per-robot payloads
	bool baked = false;	   // the context's model is the compile-time Panda
	unsigned gated = 0;	   // tasks whose generator is gated per robot and tick (refresh_otg_gating)
};

// a plain torque tick of a hierarchy with an SVD-free kernel: the only calls that advance the route
static inline bool fast_wanted(const RouteKinds& k, const TickAsk& a) { return k.fast != 0 && !a.introspection && a.do_torque && a.commit_sh; }

// The first kernel the ticks run now (observe() switches sing_mode by what the counters say; plan() may skip the SVD-free
// kernel for a while: backoff)
static inline TickForm tick_form(const TickRoute& r, const RouteSwitches& sw, const RouteKinds& k, bool baked, bool payload) {
	TickForm form;
	form.fast = k.fast;
	if (r.sing_mode && k.sing6) form.fast = k.sing6, form.sing6 = true;
	form.baked = baked;
	form.payload = payload;
	form.inlane_singular = !sw.no_inlane_singular;
	// One launch (sai2b_self.hip) for the two headline kernels without payload, while the generic kernel is the lanes-per-robot
	// one and the last look found a list of at most one round of the pass of which no wavefront holds more than one round of
	// four robots. Before any look the form is self. Speed only: each robot runs the same per-robot code either way.
	form.self = N == 7 && (form.fast == 1 || form.fast == 2) && !form.payload && sw.generic_lanes_env != 1 && !sw.no_self_serve &&
				(r.last_seen < 0 || (r.last_seen <= PASS_ROUND && r.last_wmax >= 0 && r.last_wmax <= SELF_WAVE_ROUND));
	return form;
}

// The pass ahead of the trajectory generators that tells which robots' gated tasks are active this tick: the task models of
// the current state, nothing committed. Where the SVD-free kernel for general hierarchies applies (and keeps most of the
// batch), its cascade decides for the robots it can certify and only the others take the generic kernel's range pass.
// Decided where it is launched: ahead of the tick's look, so with the back-off as the tick before left it.
struct RangePlan {
	bool run = false;
	bool cert = false;	// launch_range_cert(max_rows, payload, inlane_singular) + the 16-lane pass over its list; else
						// launch_range_pass(lanes)
	int max_rows = 0, lanes = 0;
	bool payload = false, inlane_singular = true;
};
static inline RangePlan plan_range(const TickRoute& r, const RouteSwitches& sw, const RouteKinds& k, int B, const TickAsk& a) {
	RangePlan p;
	p.run = a.do_torque && a.gated;
	if (!p.run) return p;
	p.cert = !a.introspection && r.backoff == 0 && k.cert != 0;
	p.max_rows = k.cert - 3, p.payload = a.payload, p.inlane_singular = !sw.no_inlane_singular;
	p.lanes = generic_lanes(sw, B, true);
	return p;
}

// A tick begins: true when the counts asked for LOOK_DISTANCE ticks ago are due. The caller fetches them and hands them to
// observe() (the request is taken off either way).
static inline bool look_due(TickRoute& r, const RouteKinds& k, const TickAsk& a) { return fast_wanted(k, a) && r.look.advance(); }

// What a look says about the next ticks. d: robots the SVD-free kernel declined, took: robots through its in-lane singular
// branch, wmax: most declined robots of one wavefront (-1: not known). While more than SING6_ENTER robots leave the
// hierarchy's own kernel and the hierarchy has a 4- to 6-row MotionForceTask, the 6-row kernel with the singular branch in
// the lane (until fewer than SING6_LEAVE either take that branch or leave); the generic kernel alone for BACKOFF_TICKS
// whenever a kernel for general hierarchies keeps less than 60 % of the batch. Results are the same either way.
static inline void observe(TickRoute& r, const RouteSwitches& sw, const RouteKinds& k, int B, long long d, long long took, long long wmax) {
	r.last_seen = (int)d, r.last_wmax = (int)wmax;
	const bool keeps_too_few = d * BACKOFF_DEN > (long long)B * BACKOFF_NUM;
	if (r.sing_mode) {
		if (keeps_too_few)
			r.backoff = BACKOFF_TICKS;
		else if (d + took < SING6_LEAVE && !sw.force_sing6)
			r.sing_mode = false;
	} else if (k.sing6 && d > SING6_ENTER) {
		r.sing_mode = true;
	} else if (k.fast >= 3 && keeps_too_few) {
		r.backoff = BACKOFF_TICKS;
	}
}

// everything a tick's launches need
struct TickPlan {
	TickForm form;
	TickCall call;			   // with group, and stamp != 0 when the pass (or the self form) carries the request
	bool fast_launch = false;  // an SVD-free kernel runs in front: the work list's parity flips ahead of the launch
	bool ask = false;		   // this tick asks for the work list's counts ...
	bool by_copy = false;	   // ... by two copies and an event behind the launch (the one-lane generic kernel as the pass
							   // does not take the mapped words), else by call.stamp
};
static inline TickPlan plan(TickRoute& r, const RouteSwitches& sw, const RouteKinds& k, int B, const TickAsk& a) {
	TickPlan p;
	const bool wanted = fast_wanted(k, a);
	p.form = tick_form(r, sw, k, a.baked, a.payload);  // (with the mode as this tick's look left it)
	if (wanted && p.form.fast >= 3 && r.backoff > 0) {
		r.backoff--;
		p.form.fast = 0;
	}
	p.fast_launch = wanted && p.form.fast != 0;
	p.form.self = p.form.self && p.fast_launch;
	r.last_form = !p.fast_launch ? 0 : (p.form.self ? 2 : 1);
	r.last_generic_only = a.do_torque && a.commit_sh && !p.fast_launch && !a.introspection;
	const bool long_list = p.fast_launch && r.last_seen > PASS_ROUND;
	p.call.debug = a.introspection, p.call.commit_sh = a.commit_sh, p.call.with_comp = a.with_comp, p.call.do_torque = a.do_torque;
	p.call.group = generic_lanes(sw, B, !p.fast_launch || long_list);
	// the pass over the work list reports the list's counts when asked (the lanes-per-robot pass takes the request, and so does
	// the self form, with a launch of one lane behind it; the one-lane generic kernel as the pass does not: two copies behind it)
	p.ask = p.fast_launch && !r.look.pending;
	p.by_copy = p.ask && p.call.group == 0;
	if (p.ask && !p.by_copy) {
		if (++r.stamp == 0) r.stamp = 1;
		p.call.stamp = r.stamp;
	}
	if (p.ask) {
		r.by_copy = p.by_copy;
		r.look.ask();
	}
	return p;
}

}  // namespace sai2b

// fast_block_driver.cpp — CPU-only: the FastBlock of the parameter block (csrc/sai2b_params.h) is a set of copies, and
// fast_block_fill() (csrc/sai2b_fast_block.h) is its one writer. This program includes the two headers alone, edits a DevParams
// the way the library's setters edit theirs (gains, velocity saturation, decoupling, thresholds, control frame and link, force
// space, closed-loop flags, gravity compensation, generator on / off, payload set / cleared, the measured-state copy of the
// joint sensor), fills the block as upload_params() does, and holds every value of the block to the field it copies, spelled out
// here a second time. Built with g++ under the address and undefined-behaviour sanitizers (tests/test_fast_block.py).
#include <cstdio>
#include <cstring>

#include "sai2b_fast_block.h"

using namespace sai2b;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                          \
	do {                                                                     \
		checks++;                                                            \
		if (!(cond)) {                                                       \
			failures++;                                                      \
			std::printf("FAILED %s:%d (%s): %s\n", __FILE__, __LINE__, what, #cond); \
		}                                                                    \
	} while (0)

// every value of the block against the field it copies
static void hold(const DevParams& P, const char* what) {
	const DevTask &t0 = P.task[0], &t1 = P.task[1];
	const FastBlock& f = P.fast;
	const int fl = f.entry.flags;
	CHECK(f.entry.B == P.B);
	CHECK(((fl & FB_GRAVITY_COMP) != 0) == (P.gravity_comp != 0));
	CHECK(((fl & FB_PLAIN_MOTION) != 0) == (t0.plain_motion != 0));
	CHECK(((fl & FB_USES_FORCE) != 0) == ((t0.fdim | t0.mdim) != 0));
	CHECK(((fl & FB_CL_FORCE) != 0) == (t0.cl_force != 0));
	CHECK(((fl & FB_CL_MOMENT) != 0) == (t0.cl_moment != 0));
	CHECK(((fl & FB_MFT_VSAT) != 0) == (t0.use_vsat != 0));
	CHECK(((fl & FB_JT_VSAT) != 0) == (t1.use_vsat != 0));
	CHECK(((fl & FB_MFT_BIE) != 0) == (t0.decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES));
	CHECK(((fl & FB_MFT_FULL) != 0) == (t0.decoupling == SAI2B_FULL_DYNAMIC_DECOUPLING));
	CHECK(((fl & FB_JT_BIE) != 0) == (t1.decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES));
	CHECK(((fl & FB_JT_FULL) != 0) == (t1.decoupling == SAI2B_FULL_DYNAMIC_DECOUPLING));
	CHECK(((fl & FB_JT_IMP) != 0) == (t1.decoupling == SAI2B_IMPEDANCE));
	CHECK((fl & ~((FB_JT_IMP << 1) - 1)) == 0);
	CHECK(f.entry.q == P.q && f.entry.q_again == P.q && f.entry.dq == P.dq && f.entry.tau == P.tau);
	CHECK(f.entry.law_goals0 == t0.law_goals && f.entry.state0 == t0.state && f.entry.state0_again == t0.state);
	CHECK(f.entry.istate0 == t0.istate);
	CHECK(f.entry.law_goals1 == t1.law_goals && f.entry.state1 == t1.state);
	CHECK(f.entry.payload == P.payload && f.entry.payload_link == P.payload_link);
	CHECK(std::memcmp(f.pose.frame_pos, t0.frame_pos, sizeof(t0.frame_pos)) == 0);
	CHECK(std::memcmp(f.pose.frame_rot, t0.frame_rot, sizeof(t0.frame_rot)) == 0);
	CHECK(f.pose.s_abs_tol == t0.s_abs_tol && f.pose.s_max == t0.s_max && f.pose.link == t0.link);
	CHECK(f.law.dt == t0.dt);
	CHECK(std::memcmp(f.law.kp_pos, t0.kp_pos, 24) == 0 && std::memcmp(f.law.kv_pos, t0.kv_pos, 24) == 0);
	CHECK(std::memcmp(f.law.ki_pos, t0.ki_pos, 24) == 0 && std::memcmp(f.law.kp_ori, t0.kp_ori, 24) == 0);
	CHECK(std::memcmp(f.law.kv_ori, t0.kv_ori, 24) == 0 && std::memcmp(f.law.ki_ori, t0.ki_ori, 24) == 0);
	CHECK(f.chain.bie_threshold == (t1.decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES ? t1.bie_threshold : t0.bie_threshold));
	CHECK(f.jt.dt == t1.dt && f.jt.use_vsat == t1.use_vsat);
	CHECK(std::memcmp(f.jt.kp, t1.kp, sizeof(t1.kp)) == 0 && std::memcmp(f.jt.kv, t1.kv, sizeof(t1.kv)) == 0);
	CHECK(std::memcmp(f.jt.ki, t1.ki, sizeof(t1.ki)) == 0 && std::memcmp(f.jt.vsat, t1.vsat, sizeof(t1.vsat)) == 0);
}

// a change as a setter makes it, then what upload_params() does; the block must follow, and only through the fill
template <class F>
static void change(DevParams& P, const char* what, F&& edit) {
	const FastBlock before = P.fast;
	edit(P);
	CHECK(std::memcmp(&before, &P.fast, sizeof(FastBlock)) == 0);  // (no edit above reaches into the block)
	fast_block_fill(P);
	hold(P, what);
	DevParams again = P;  // filling twice changes nothing: the block depends on nothing but the fields above it
	fast_block_fill(again);
	CHECK(std::memcmp(&again.fast, &P.fast, sizeof(FastBlock)) == 0);
}

int main() {
	const char* what = "layout";
	CHECK(offsetof(DevParams, fast) % 64 == 0 && sizeof(FastBlock) % 64 == 0);
	CHECK(offsetof(DevParams, fast) + sizeof(FastBlock) == sizeof(DevParams));	// behind everything else
	CHECK(offsetof(FastBlock, entry) == 0 && sizeof(FastEntry) == 128 && offsetof(FastEntry, tau) == 64);
	CHECK(offsetof(FastBlock, pose) % 64 == 0 && offsetof(FastBlock, law) % 64 == 0 && offsetof(FastBlock, chain) % 64 == 0 &&
		  offsetof(FastBlock, jt) % 64 == 0);

	static DevParams P;	 // (zero-initialised, as create_impl's memset leaves it)
	static double buf[64];
	static int ibuf[8];
	P.B = 130, P.n_tasks = 2;
	P.q = buf, P.dq = buf + 1, P.tau = buf + 2;
	DevTask &t0 = P.task[0], &t1 = P.task[1];
	t0.type = SAI2B_MOTION_FORCE_TASK, t1.type = SAI2B_JOINT_TASK;
	t0.goals = buf + 3, t0.otg_desired = buf + 4, t0.law_goals = t0.goals, t0.state = buf + 5, t0.istate = ibuf;
	t1.goals = buf + 6, t1.otg_state = buf + 7, t1.law_goals = t1.goals, t1.state = buf + 8;
	t0.dt = t1.dt = 0.001, t0.link = N - 1, t0.plain_motion = 1;
	t0.frame_rot[0] = t0.frame_rot[4] = t0.frame_rot[8] = 1;
	t0.s_abs_tol = 1e-3, t0.s_max = 6e-2;
	t0.decoupling = t1.decoupling = SAI2B_BOUNDED_INERTIA_ESTIMATES, t0.bie_threshold = t1.bie_threshold = 0.1;
	for (int k = 0; k < 3; k++) t0.kp_pos[k] = 100 + k, t0.kv_pos[k] = 20 + k, t0.kp_ori[k] = 200 + k, t0.kv_ori[k] = 30 + k;
	for (int i = 0; i < N; i++) t1.kp[i] = 50 + i, t1.kv[i] = 14 + i, t1.vsat[i] = 1.0 + i;
	change(P, "as created", [](DevParams&) {});

	change(P, "MotionForceTask gains", [](DevParams& p) {
		for (int k = 0; k < 3; k++) {
			p.task[0].kp_pos[k] = 7 + k, p.task[0].kv_pos[k] = 8 + k, p.task[0].ki_pos[k] = 9 + k;
			p.task[0].kp_ori[k] = 10 + k, p.task[0].kv_ori[k] = 11 + k, p.task[0].ki_ori[k] = 12 + k;
		}
	});
	change(P, "JointTask gains", [](DevParams& p) {
		for (int i = 0; i < N; i++) p.task[1].kp[i] = 3 + i, p.task[1].kv[i] = 4 + i, p.task[1].ki[i] = 5 + i;
	});
	change(P, "control period", [](DevParams& p) { p.task[0].dt = 0.002, p.task[1].dt = 0.004; });
	change(P, "JointTask velocity saturation on", [](DevParams& p) {
		p.task[1].use_vsat = 1;
		for (int i = 0; i < N; i++) p.task[1].vsat[i] = 0.25 * (i + 1);
	});
	change(P, "JointTask velocity saturation off", [](DevParams& p) { p.task[1].use_vsat = 0; });
	change(P, "MotionForceTask velocity saturation on", [](DevParams& p) { p.task[0].use_vsat = 1, p.task[0].plain_motion = 0; });
	change(P, "MotionForceTask velocity saturation off", [](DevParams& p) { p.task[0].use_vsat = 0, p.task[0].plain_motion = 1; });
	const int modes[3] = {SAI2B_BOUNDED_INERTIA_ESTIMATES, SAI2B_FULL_DYNAMIC_DECOUPLING, SAI2B_IMPEDANCE};
	for (int a = 0; a < 3; a++)
		for (int b = 0; b < 3; b++)
			change(P, "decoupling modes", [&](DevParams& p) { p.task[0].decoupling = modes[a], p.task[1].decoupling = modes[b]; });
	change(P, "thresholds, JointTask bounded-inertia", [](DevParams& p) {
		p.task[0].decoupling = SAI2B_FULL_DYNAMIC_DECOUPLING, p.task[1].decoupling = SAI2B_BOUNDED_INERTIA_ESTIMATES;
		p.task[0].bie_threshold = 0.3, p.task[1].bie_threshold = 0.2;
	});
	change(P, "thresholds, MotionForceTask bounded-inertia", [](DevParams& p) {
		p.task[0].decoupling = SAI2B_BOUNDED_INERTIA_ESTIMATES, p.task[1].decoupling = SAI2B_IMPEDANCE;
	});
	change(P, "singularity bounds", [](DevParams& p) { p.task[0].s_abs_tol = 2e-3, p.task[0].s_max = 0.1; });
	change(P, "control frame and link", [](DevParams& p) {
		p.task[0].link = 3;
		for (int k = 0; k < 3; k++) p.task[0].frame_pos[k] = 0.1 * (k + 1);
		const double R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
		std::memcpy(p.task[0].frame_rot, R, sizeof(R));
	});
	change(P, "force space", [](DevParams& p) { p.task[0].fdim = 1, p.task[0].plain_motion = 0; });
	change(P, "moment space only", [](DevParams& p) { p.task[0].fdim = 0, p.task[0].mdim = 2; });
	change(P, "closed-loop force", [](DevParams& p) { p.task[0].cl_force = 1; });
	change(P, "closed-loop moment", [](DevParams& p) { p.task[0].cl_force = 0, p.task[0].cl_moment = 1; });
	change(P, "no force space again", [](DevParams& p) { p.task[0].mdim = 0, p.task[0].cl_moment = 0, p.task[0].plain_motion = 1; });
	change(P, "gravity compensation on", [](DevParams& p) { p.gravity_comp = 1; });
	change(P, "gravity compensation off", [](DevParams& p) { p.gravity_comp = 0; });
	change(P, "generators on", [](DevParams& p) {
		p.task[0].otg_on = 1, p.task[0].law_goals = p.task[0].otg_desired;
		p.task[1].otg_on = 1, p.task[1].otg_out_is_desired = 1, p.task[1].law_goals = p.task[1].otg_state + (size_t)OTG_OUT * p.B;
	});
	change(P, "generators off", [](DevParams& p) {
		p.task[0].otg_on = 0, p.task[0].law_goals = p.task[0].goals;
		p.task[1].otg_on = 0, p.task[1].law_goals = p.task[1].goals;
	});
	change(P, "payload set", [](DevParams& p) { p.payload = buf + 9, p.payload_link = 3; });
	change(P, "payload cleared", [](DevParams& p) { p.payload = nullptr, p.payload_link = 0; });
	// the joint sensor's copy of the parameters: the same block with the measured pair as its state
	DevParams meas = P;
	change(meas, "measured state", [](DevParams& p) { p.q = buf + 10, p.dq = buf + 11; });
	what = "measured state";
	CHECK(P.fast.entry.q == P.q && meas.fast.entry.q == buf + 10 && meas.fast.entry.q_again == buf + 10 && meas.fast.entry.dq == buf + 11);

	if (failures) {
		std::printf("%d of %d checks failed\n", failures, checks);
		return 1;
	}
	std::printf("ok %d\n", checks);
	return 0;
}

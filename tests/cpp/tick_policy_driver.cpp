// tick_policy_driver.cpp — the host's tick routing (csrc/sai2b_tick_policy.h) on a CPU: hand-built hierarchies and scripted
// counts, checked tick by tick. Built by tests/test_tick_policy.py with -DSAI2B_N=7 and 6. Prints one line per failed check
// and "ok <checks>" at the end; exit status 1 when a check failed.
#include <cstdio>

#include "sai2b_tick_policy.h"

using namespace sai2b;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                      \
	do {                                                                 \
		g_checks++;                                                      \
		if (!(cond)) {                                                   \
			g_failed++;                                                  \
			std::printf("FAILED line %d (N = %d): %s\n", __LINE__, N, #cond); \
		}                                                                \
	} while (0)

// a hierarchy built task by task
struct Robot {
	DevParams hp = {};
	sai2b_task_config cfg[SAI2B_MAX_TASKS] = {};
	int joint_type[SAI2B_MAX_DOF] = {};	 // all revolute
	int T = 0;
	Robot& mft(int rank, bool full_projection, bool passivity = false, bool closed_loop = false) {
		cfg[T].type = hp.task[T].type = SAI2B_MOTION_FORCE_TASK;
		cfg[T].passivity_enabled = passivity, cfg[T].closed_loop_force = closed_loop;
		hp.task[T].rank = rank, hp.task[T].full_projection = full_projection;
		hp.n_tasks = ++T;
		return *this;
	}
	Robot& jt(int k0, bool full_selection) {
		cfg[T].type = hp.task[T].type = SAI2B_JOINT_TASK;
		hp.task[T].k0 = k0, hp.task[T].full_selection = full_selection;
		hp.n_tasks = ++T;
		return *this;
	}
	Robot& prismatic(int joint) {
		joint_type[joint] = SAI2B_PRISMATIC;
		return *this;
	}
	Hierarchy h() const { return Hierarchy{&hp, cfg, T, joint_type}; }
	RouteKinds kinds(const RouteSwitches& sw = RouteSwitches()) const { return route_kinds(sw, h()); }
};

// a context's route, driven as launch_tick drives it: the range pass is planned first, then the look, then the tick
struct Sim {
	RouteSwitches sw;
	RouteKinds k;
	int B;
	TickRoute r;
	TickAsk a;
	RangePlan range;
	bool looked = false;
	Sim(const RouteSwitches& sw_, const RouteKinds& k_, int B_) : sw(sw_), k(k_), B(B_), r(sw_) {}
	// one tick; d / took / wmax: what the device answers if this tick looks
	TickPlan tick(long long d = 0, long long took = 0, long long wmax = 0) {
		range = plan_range(r, sw, k, B, a);
		looked = look_due(r, k, a);
		if (looked) observe(r, sw, k, B, d, took, wmax);
		return plan(r, sw, k, B, a);
	}
	// ticks up to and including the next one that looks, which sees these counts
	TickPlan look(long long d, long long took, long long wmax) {
		for (int i = 0; i < 4 * LOOK_DISTANCE; i++) {
			const TickPlan p = tick(d, took, wmax);
			if (looked) return p;
		}
		CHECK(!"no look within 32 ticks");
		return TickPlan();
	}
};

static RouteSwitches with(void (*set)(RouteSwitches&)) {
	RouteSwitches sw;
	set(sw);
	return sw;
}

static void eligibility() {
	const RouteSwitches none;
	const Robot headline1 = Robot().mft(6, true), headline2 = Robot().mft(6, true).jt(N, true);
	// rows 6, slots N + 12 + N (7 + 12 + 7 = 26 on the Panda): the 6-row instantiation
	CHECK(headline1.kinds().cert == 9 && headline2.kinds().cert == 9);
	CHECK(headline2.kinds().sing6 == 9);
	if (N == 7) {
		CHECK(headline1.kinds().fast == 1);
		CHECK(headline2.kinds().fast == 2);
		CHECK(headline2.kinds(with([](RouteSwitches& s) { s.prefer_cert = true; })).fast == 9);
		CHECK(Robot().mft(6, true).jt(N, true).prismatic(2).kinds().fast == 9);
		// behind a full MotionForceTask only a full JointTask is the headline's
		CHECK(Robot().mft(6, true).jt(1, false).kinds().fast == 3 + 6);
		CHECK(Robot().mft(5, false).jt(2, false).kinds().fast == 3 + 5);
	} else {
		CHECK(headline1.kinds().fast == 9);
		CHECK(headline2.kinds().fast == 9);
	}
	CHECK(Robot().mft(3, false).jt(2, false).kinds().cert == 3 + 3);
	CHECK(Robot().mft(3, false).jt(2, false).kinds().sing6 == 0);	 // no 4- to 6-row task
	CHECK(Robot().mft(2, false).jt(4, false).kinds().sing6 == 3 + 4);
	const RouteKinds off1 = headline2.kinds(with([](RouteSwitches& s) { s.no_fast_path = true; }));
	CHECK(off1.cert == 0 && off1.fast == 0 && off1.sing6 == 0);
	const RouteKinds off2 = headline2.kinds(with([](RouteSwitches& s) { s.no_cert_path = true; }));
	CHECK(off2.cert == 0 && off2.sing6 == 0 && off2.fast == (N == 7 ? 2 : 0));
	CHECK(headline2.kinds(with([](RouteSwitches& s) { s.no_sing6 = true; })).sing6 == 0);
	CHECK(headline2.kinds(with([](RouteSwitches& s) { s.no_inlane_singular = true; })).sing6 == 0);
	// not eligible at all
	const Robot refused[] = {
		Robot().mft(6, true, /*passivity=*/true, /*closed_loop=*/true),	 // the observer mutates state inside the law
		Robot().jt(N, true).mft(3, false),								 // a full JointTask not at the bottom
		Robot().mft(6, true).jt(N - 5, false),							 // rows 6 + N - 5 > N
		Robot().mft(2, false).mft(2, false).mft(1, false),				 // slots N + 36 > 36
	};
	for (const Robot& rb : refused) CHECK(rb.kinds().cert == 0 && rb.kinds().fast == 0 && rb.kinds().sing6 == 0);
	CHECK(Robot().mft(6, true, true, false).kinds().cert == 9);	 // passivity alone does not refuse
	if (N >= 7) {
		const RouteKinds k7 = Robot().jt(7, false).kinds();	 // a partial task of more than 6 rows
		CHECK(k7.cert == 0 && k7.fast == 0);
	}
	CHECK(Robot().jt(6, false).kinds().cert == 3 + 6);

	// one task on its own
	for (int rank = 0; rank <= 6; rank++) CHECK(task_cert_rows(none, Robot().mft(rank, rank == 6).h(), 0, false) == rank);
	CHECK(task_cert_rows(none, Robot().mft(6, true, true, true).h(), 0, false) == 0);
	CHECK(task_cert_rows(none, headline2.h(), 1, false) == 1);	// a full JointTask: the small instantiation
	for (int k0 = 1; k0 <= 6 && k0 <= N; k0++) CHECK(task_cert_rows(none, Robot().mft(1, false).jt(k0, false).h(), 1, false) == k0);
	if (N >= 7) CHECK(task_cert_rows(none, Robot().jt(7, false).h(), 0, false) == 0);
	CHECK(task_cert_rows(none, headline2.h(), 0, /*introspection=*/true) == 0);
	CHECK(task_cert_rows(with([](RouteSwitches& s) { s.no_task_cert = true; }), headline2.h(), 0, false) == 0);
	CHECK(task_cert_rows(with([](RouteSwitches& s) { s.no_fast_path = true; }), headline2.h(), 0, false) == 0);
	CHECK(task_cert_rows(with([](RouteSwitches& s) { s.no_cert_path = true; }), headline2.h(), 0, false) == 0);
	CHECK(task_cert_rows(with([](RouteSwitches& s) { s.prefer_cert = true; }), headline2.h(), 0, false) == 6);

	// lanes per robot of the generic kernel
	CHECK(generic_lanes(none, 16383, true) == 16 && generic_lanes(none, 16384, true) == 8 && generic_lanes(none, 65536, false) == 16);
	RouteSwitches lanes;
	lanes.generic_lanes_env = 1;
	CHECK(generic_lanes(lanes, 65536, true) == 0 && generic_lanes(lanes, 64, false) == 0);
	lanes.generic_lanes_env = 8;
	CHECK(generic_lanes(lanes, 64, false) == 8);
	lanes.generic_lanes_env = 16;
	CHECK(generic_lanes(lanes, 65536, true) == 16);
	lanes.generic_lanes_env = 4;  // not a form of the kernel: as unset
	CHECK(generic_lanes(lanes, 65536, true) == 8);
}

// the hierarchy of the headline tick: fast = 2 on the Panda, the kernel for general hierarchies (9) elsewhere
static const Robot& headline() {
	static const Robot rb = Robot().mft(6, true).jt(N, true);
	return rb;
}

static void asking() {
	Sim s(RouteSwitches(), headline().kinds(), 130);
	CHECK(s.r.pending() == 0 && s.r.last_seen == -1 && s.r.last_wmax == -1);
	TickPlan p = s.tick();
	CHECK(!s.looked && p.ask && !p.by_copy && p.call.stamp == 1 && p.fast_launch && s.r.pending() == 1);
	CHECK(p.call.group == 16 && !p.call.debug && p.call.commit_sh && p.call.with_comp && p.call.do_torque);
	for (int t = 2; t <= 8; t++) {
		p = s.tick();
		CHECK(!s.looked && !p.ask && p.call.stamp == 0 && p.fast_launch && s.r.pending() == 1);
	}
	p = s.tick(3, 1, 2);  // tick 9
	CHECK(s.looked && s.r.last_seen == 3 && s.r.last_wmax == 2);
	CHECK(p.ask && !p.by_copy && p.call.stamp == 2 && s.r.pending() == 1);
	for (int t = 10; t <= 16; t++) CHECK(!s.tick().ask && !s.looked);
	p = s.tick(0, 0, 0);  // tick 17
	CHECK(s.looked && p.ask && p.call.stamp == 3 && s.r.last_seen == 0);

	// the stamp wraps past 0
	s.r.stamp = 0xFFFFFFFEu;
	p = s.look(0, 0, 0);
	CHECK(p.ask && p.call.stamp == 0xFFFFFFFFu);
	p = s.look(0, 0, 0);
	CHECK(p.ask && p.call.stamp == 1);

	// the one-lane generic kernel as the pass: by copies
	RouteSwitches one;
	one.generic_lanes_env = 1;
	Sim c(one, headline().kinds(one), 130);
	p = c.tick();
	CHECK(p.ask && p.by_copy && p.call.stamp == 0 && p.call.group == 0 && c.r.pending() == 2 && c.r.stamp == 0);
	CHECK(!p.form.self && c.r.last_form == 1);
	for (int t = 2; t <= 8; t++) CHECK(!c.tick().ask && c.r.pending() == 2);
	p = c.tick(50, 0, -1);
	CHECK(c.looked && p.ask && p.by_copy && !p.form.self && c.r.last_seen == 50 && c.r.last_wmax == -1 && c.r.pending() == 2);
}

static void form_of_the_tick() {
	const RouteSwitches none;
	const bool panda = N == 7;	// the one-launch form exists for the two headline kernels only
	const int two = 1, self = panda ? 2 : 1;
	{
		Sim s(none, headline().kinds(), 65536);
		TickPlan p = s.tick();	// before any look
		CHECK(p.form.self == panda && s.r.last_form == self && p.form.fast == (panda ? 2 : 9) && !p.form.sing6);
		CHECK(p.form.inlane_singular && !p.form.payload && !p.form.baked);
		p = s.look(100, 0, 2);
		CHECK(p.form.self == panda && s.r.last_form == self && p.call.group == 16);
		p = s.look(100, 0, 4);
		CHECK(p.form.self == panda && s.r.last_form == self);
		p = s.look(100, 0, 5);	// more than one round of four in one wavefront
		CHECK(!p.form.self && s.r.last_form == two && p.call.group == 16 && p.fast_launch);
		p = s.look(4096, 0, 1);
		CHECK(p.form.self == panda && p.call.group == 16);
		p = s.look(4097, 0, 1);	 // more than one round of the pass
		CHECK(!p.form.self && s.r.last_form == two && p.call.group == 8);
		p = s.look(5000, 0, 1);
		CHECK(!p.form.self && s.r.last_form == two && p.call.group == 8 && p.fast_launch);
		p = s.look(100, 0, -1);	 // the third word not known
		CHECK(!p.form.self && s.r.last_form == two && p.call.group == 16);
		p = s.look(0, 0, 0);
		CHECK(p.form.self == panda && s.r.last_form == self);
	}
	{
		Sim s(none, headline().kinds(), 8192);	// a long list of a small batch: 16 lanes still
		const TickPlan p = s.look(5000, 0, 1);
		CHECK(!p.form.self && p.call.group == 16);
		// (more than 40 % of this batch: a kernel for general hierarchies rests, the headline kernels do not)
		CHECK(s.r.last_form == (panda ? two : 0) && p.fast_launch == panda);
	}
	{
		Sim s(none, headline().kinds(), 65536);
		s.a.payload = true, s.a.baked = true;
		const TickPlan p = s.tick();
		CHECK(!p.form.self && p.form.payload && p.form.baked && s.r.last_form == two && p.ask && p.call.stamp == 1);
	}
	{
		const RouteSwitches sw = with([](RouteSwitches& x) { x.no_self_serve = true; });
		Sim s(sw, headline().kinds(sw), 65536);
		CHECK(!s.tick().form.self && s.r.last_form == two);
		CHECK(!s.look(0, 0, 0).form.self && s.r.last_form == two);
	}
	{
		const RouteSwitches sw = with([](RouteSwitches& x) { x.no_fast_path = true; });
		Sim s(sw, headline().kinds(sw), 65536);	 // no SVD-free kernel: the generic one for the whole batch, 8 lanes
		const TickPlan p = s.tick();
		CHECK(!p.fast_launch && p.form.fast == 0 && !p.form.self && s.r.last_form == 0 && s.r.last_generic_only && p.call.group == 8 && !p.ask);
		CHECK(s.r.look.tick == 0);
	}
	{
		const RouteSwitches sw = with([](RouteSwitches& x) { x.no_inlane_singular = true; });
		Sim s(sw, headline().kinds(sw), 64);
		CHECK(!s.tick().form.inlane_singular);
	}
}

static void singular_mode() {
	const int B = 65536;
	const RouteSwitches none;
	const int own = N == 7 ? 2 : 9;	 // the hierarchy's own first kernel
	{
		Sim s(none, headline().kinds(), B);
		TickPlan p = s.look(20480, 0, 1);
		CHECK(!s.r.sing_mode && p.form.fast == own && !p.form.sing6);
		p = s.look(20481, 0, 1);
		CHECK(s.r.sing_mode && p.form.fast == 9 && p.form.sing6 && !p.form.self && p.fast_launch && s.r.last_form == 1 && s.r.backoff == 0);
		p = s.look(15360, 0, 1);
		CHECK(s.r.sing_mode && p.form.sing6);
		p = s.look(360, 15000, 1);
		CHECK(s.r.sing_mode && p.form.sing6);
		p = s.look(359, 15000, 1);
		CHECK(!s.r.sing_mode && !p.form.sing6 && p.form.fast == own);
		p = s.look(20481, 0, 1);
		CHECK(s.r.sing_mode);
		p = s.look(15359, 0, 1);
		CHECK(!s.r.sing_mode);
		// inside the mode the 6-row kernel is one for general hierarchies: it rests when it keeps less than 60 %
		s.look(26214, 0, 1);
		CHECK(s.r.sing_mode && s.r.backoff == 0);
		p = s.look(26215, 0, 1);
		CHECK(s.r.sing_mode && p.form.fast == 0 && !p.fast_launch && s.r.backoff == BACKOFF_TICKS - 1 && s.r.last_generic_only);
	}
	{
		const RouteSwitches sw = with([](RouteSwitches& x) { x.force_sing6 = true; });
		Sim s(sw, headline().kinds(sw), B);
		TickPlan p = s.tick();
		CHECK(s.r.sing_mode && p.form.fast == 9 && p.form.sing6 && !p.form.self);
		p = s.look(0, 0, 0);
		CHECK(s.r.sing_mode && p.form.sing6);
	}
	{
		const RouteSwitches sw = with([](RouteSwitches& x) { x.no_sing6 = true; });
		Sim s(sw, headline().kinds(sw), B);
		const TickPlan p = s.look(30000, 0, 1);
		CHECK(!s.r.sing_mode && !p.form.sing6);
		// the headline kernels never rest; the kernel for general hierarchies does
		CHECK(p.form.fast == (N == 7 ? own : 0));
		CHECK(s.r.backoff == (N == 7 ? 0 : BACKOFF_TICKS - 1));
		CHECK(p.fast_launch == (N == 7));
	}
}

static void back_off() {
	// [3-row MFT, 2-row JT]: the kernel for general hierarchies, no 6-row alternative
	const Robot rb = Robot().mft(3, false).jt(2, false);
	const RouteKinds k = rb.kinds();
	CHECK(k.fast == 6 && k.cert == 6 && k.sing6 == 0);
	Sim s(RouteSwitches(), k, 1000);
	s.a.gated = 2;	// the JointTask's generator is gated: a range pass every tick
	TickPlan p = s.look(400, 0, 0);	 // 400 * 5 = 2 * 1000: keeps 60 %
	CHECK(s.r.backoff == 0 && p.fast_launch && p.form.fast == 6 && s.range.run && s.range.cert && s.range.max_rows == 3);
	CHECK(s.range.inlane_singular && !s.range.payload);
	const long long before = s.r.look.tick;
	p = s.look(401, 0, 0);
	CHECK(s.r.look.tick == before + LOOK_DISTANCE);
	// the look's own tick: its range pass was planned ahead of the look
	CHECK(s.range.run && s.range.cert);
	int generic = 0, range_generic = 0;
	for (;; p = s.tick(999, 999, 999)) {
		if (p.fast_launch) break;
		generic++;
		CHECK(p.form.fast == 0 && !p.form.self && !p.ask && p.call.stamp == 0 && s.looked == (generic == 1));
		CHECK(s.r.last_generic_only && s.r.last_form == 0 && s.r.pending() == 0 && p.call.group == 16);
		CHECK(s.r.backoff == BACKOFF_TICKS - generic);
		if (generic > 1) {
			CHECK(s.range.run && !s.range.cert && s.range.lanes == 16);
			range_generic++;
		}
		if (generic > 2 * BACKOFF_TICKS) break;
	}
	CHECK(generic == BACKOFF_TICKS && range_generic == BACKOFF_TICKS - 1);
	// the SVD-free kernel again, asking on its first tick
	CHECK(p.fast_launch && p.form.fast == 6 && p.ask && p.call.stamp != 0 && !s.looked && s.range.cert && !s.r.last_generic_only);
	CHECK(s.r.look.tick == before + LOOK_DISTANCE + BACKOFF_TICKS);	 // (the ticks of a back-off count)
	// introspection: the range pass is the generic kernel's
	s.a.introspection = true;
	s.tick();
	CHECK(s.range.run && !s.range.cert);
	s.a.introspection = false, s.a.gated = 0;
	s.tick();
	CHECK(!s.range.run);
	s.a.gated = 2, s.a.do_torque = 0;
	s.tick();
	CHECK(!s.range.run);
	// a whole batch of 16 384 robots takes 8 lanes
	Sim big(RouteSwitches(), k, 16384);
	big.a.gated = 2;
	big.r.backoff = 1;
	big.tick();
	CHECK(big.range.run && !big.range.cert && big.range.lanes == 8);
}

static void calls_that_do_not_advance() {
	for (int which = 0; which < 3; which++) {
		Sim s(RouteSwitches(), headline().kinds(), 130);
		s.tick();
		const TickRoute before = s.r;
		if (which == 0) s.a.introspection = true;
		if (which == 1) s.a.do_torque = 0;
		if (which == 2) s.a.commit_sh = 0;
		for (int t = 0; t < 2 * LOOK_DISTANCE; t++) {
			const TickPlan p = s.tick(7, 7, 7);
			CHECK(!p.fast_launch && !p.form.self && !p.ask && !p.by_copy && p.call.stamp == 0 && !s.looked);
			CHECK(p.call.debug == (which == 0) && p.call.do_torque == (which != 1) && p.call.commit_sh == (which != 2));
			CHECK(s.r.look.tick == before.look.tick && s.r.look.pending && s.r.stamp == before.stamp && s.r.last_seen == -1);
			CHECK(s.r.last_form == 0 && !s.r.last_generic_only);
		}
		s.a = TickAsk();
		for (int t = 2; t <= 8; t++) CHECK(!s.tick().ask && !s.looked);
		CHECK(s.tick(1, 0, 1).ask && s.looked);	 // the ninth tick that wants the SVD-free kernel
	}
}

// the generators' busy count uses the same clock
static void delayed_look() {
	DelayedLook l;
	CHECK(!l.advance() && l.tick == 1);
	l.ask();
	for (int t = 2; t <= 8; t++) CHECK(!l.advance() && l.pending);
	CHECK(l.advance() && !l.pending && l.tick == 9);
	CHECK(!l.advance());
	l.ask();
	for (int t = 0; t < LOOK_DISTANCE - 1; t++) CHECK(!l.advance());
	CHECK(l.advance());
}

int main() {
	eligibility();
	asking();
	form_of_the_tick();
	singular_mode();
	back_off();
	calls_that_do_not_advance();
	delayed_look();
	if (g_failed) {
		std::printf("%d of %d checks FAILED\n", g_failed, g_checks);
		return 1;
	}
	std::printf("ok %d\n", g_checks);
	return 0;
}

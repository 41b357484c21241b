// sai2b_fast_block.h — the one writer of DevParams::fast (FastBlock, sai2b_params.h). Host code only, no HIP: upload_params()
// calls it on every copy of the parameters it is about to send (sai2b_host.cpp), so whatever a setter changed in DevParams or
// in a DevTask, the pointers a generator switches (law_goals) and the measured state of the joint-sensor copy included, is in
// the block before a kernel can read it. tests/cpp/fast_block_driver.cpp holds it to the fields it copies.
#pragma once
#include <cstring>

#include "sai2b_params.h"

namespace sai2b {

inline void fast_block_fill(DevParams& P) {
	const DevTask &t0 = P.task[0], &t1 = P.task[1];
	FastBlock& f = P.fast;
	std::memset(&f, 0, sizeof(f));	// the padding too: the block is compared and uploaded as bytes
	FastEntry& e = f.entry;
	e.B = P.B;
	e.flags = (P.gravity_comp ? FB_GRAVITY_COMP : 0) | (t0.plain_motion ? FB_PLAIN_MOTION : 0) |
			  ((t0.fdim | t0.mdim) != 0 ? FB_USES_FORCE : 0) | (t0.cl_force ? FB_CL_FORCE : 0) | (t0.cl_moment ? FB_CL_MOMENT : 0) |
			  (t0.use_vsat ? FB_MFT_VSAT : 0) | (t1.use_vsat ? FB_JT_VSAT : 0) |
			  (t0.decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES ? FB_MFT_BIE : 0) |
			  (t0.decoupling == SAI2B_FULL_DYNAMIC_DECOUPLING ? FB_MFT_FULL : 0) |
			  (t1.decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES ? FB_JT_BIE : 0) |
			  (t1.decoupling == SAI2B_FULL_DYNAMIC_DECOUPLING ? FB_JT_FULL : 0) | (t1.decoupling == SAI2B_IMPEDANCE ? FB_JT_IMP : 0);
	e.q = e.q_again = P.q, e.dq = P.dq, e.tau = P.tau;
	e.law_goals0 = t0.law_goals, e.state0 = e.state0_again = t0.state, e.istate0 = t0.istate;
	e.law_goals1 = t1.law_goals, e.state1 = t1.state;
	e.payload = P.payload, e.payload_link = P.payload_link;
	FastPose& p = f.pose;
	std::memcpy(p.frame_pos, t0.frame_pos, sizeof(p.frame_pos));
	std::memcpy(p.frame_rot, t0.frame_rot, sizeof(p.frame_rot));
	p.s_abs_tol = t0.s_abs_tol, p.s_max = t0.s_max, p.link = t0.link;
	FastLaw& l = f.law;
	l.dt = t0.dt;
	for (int k = 0; k < 3; k++) {
		l.kp_pos[k] = t0.kp_pos[k], l.kv_pos[k] = t0.kv_pos[k], l.ki_pos[k] = t0.ki_pos[k];
		l.kp_ori[k] = t0.kp_ori[k], l.kv_ori[k] = t0.kv_ori[k], l.ki_ori[k] = t0.ki_ori[k];
	}
	f.chain.bie_threshold = t1.decoupling == SAI2B_BOUNDED_INERTIA_ESTIMATES ? t1.bie_threshold : t0.bie_threshold;
	FastJt& j = f.jt;
	j.dt = t1.dt, j.use_vsat = t1.use_vsat;
	for (int i = 0; i < N; i++) j.kp[i] = t1.kp[i], j.kv[i] = t1.kv[i], j.ki[i] = t1.ki[i], j.vsat[i] = t1.vsat[i];
}

}  // namespace sai2b

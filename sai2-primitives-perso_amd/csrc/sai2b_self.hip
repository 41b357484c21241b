// sai2b_self.hip — the headline tick as ONE launch: the SVD-free body of tick_fast_kernel (sai2b_fast_body.hpp), and behind it,
// in the same wavefront, the lanes-per-robot generic tick (sai2b_group_tick.hpp) for the robots this wavefront declined.
// There is no work list and no protocol between workgroups: a wavefront without declined robots executes a ballot and a
// branch behind the fast body, nothing else. The host chooses this form while wavefronts decline few robots (launch_tick in
// sai2b_host.cpp); every robot runs the same per-robot code as in the two-launch form.
#include <hip/hip_runtime.h>

#if SAI2B_N == 7
#include "sai2b_fast_body.hpp"
#include "sai2b_group_tick.hpp"
#endif
#include "sai2b_launch.h"

namespace sai2b {

#if SAI2B_N == 7
// Pp / P2p: the same parameter block twice. The fast body reads it through the restrict pointer, as in tick_fast_kernel; the
// tail reads it through the plain one. With the restrict pointer handed on to the tail, the body's reads of the block turn into
// vector loads inside the DMA window and retire the DMA early (tests/test_self_serve_isa.py holds the window).
// fb_counts as tick_fast_kernel: [parity] += declined robots, one atomic per wavefront that has any; [4 + parity] = the largest
// number of them in one wavefront (the host leaves this form when a wavefront needs more than one round); the other parity's
// words are cleared for the next tick. No list is written.
template <int FAST, bool BAKED>
__global__ __launch_bounds__(64) void tick_self_kernel(const DevParams* __restrict__ Pp, const DevParams* P2p, int with_comp,
														  int* __restrict__ fb_counts, int parity) {
	constexpr int GPB = 4;	// 16 lanes per robot: four robots per round
	constexpr int PADS = GPB * grp::PAD_DOUBLES;
	constexpr int IMG = FAST == 2 ? StageLayout<2>::DOUBLES : PADS;
	static_assert(IMG >= PADS, "the groups' pads alias the start of the image");
	__shared__ real img[IMG];
	const int b0 = blockIdx.x * 64;
	if (blockIdx.x == 0 && threadIdx.x == 0)
		((gint*)fb_counts)[1 - parity] = 0, ((gint*)fb_counts)[2 + (1 - parity)] = 0, ((gint*)fb_counts)[4 + (1 - parity)] = 0;
	bool out;
	if constexpr (FAST == 1) {
		const int b = b0 + threadIdx.x;
		out = b < Pp->B ? tick_fast1_loads<BAKED, NoPayload, true>(*Pp, with_comp, fb_counts, nullptr, parity, b) : false;
	} else {
		out = tick_fast_body<FAST, BAKED, NoPayload, true>(Pp, with_comp, fb_counts, nullptr, parity, img);
	}
	unsigned long long rest = __ballot(out);
	if (!rest) return;
	if (threadIdx.x == 0) {
		atomicAdd(&fb_counts[parity], __popcll(rest));
		atomicMax(&fb_counts[4 + parity], __popcll(rest));
	}
	// every read of the image and of the parked M / g lies before this point: the pads may overwrite them from here
	__syncthreads();
	const DevParams& P2 = *P2p;
	const int gi = grp::group<16>();
	real* pad = img + gi * grp::PAD_DOUBLES;
#pragma unroll 1
	while (rest) {
		// group gi takes the gi-th lowest robot that is left (uniform inside a group, as tick_group_kernel's list entries)
		unsigned long long m = rest;
		UNROLL for (int k = 0; k < GPB - 1; k++) m &= k < gi ? m - 1 : ~0ull;
		if (m) grp::tick_robot<16, false>(P2, b0 + __ffsll(m) - 1, pad, 1, with_comp, 1);
		UNROLL for (int k = 0; k < GPB; k++) rest &= rest - 1;
	}
}

// The counts of a self-form tick for the host, when it asks (TickCall::stamp): what tick_group_kernel's workgroup 0 writes in
// the two-launch form, as a launch of one lane behind the tick. count = fb_counts + parity.
__global__ void worklist_report_kernel(const int* __restrict__ count, unsigned long long* report, unsigned stamp) {
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	const unsigned long long tag = (unsigned long long)stamp << 32;
	__hip_atomic_store(report, tag | (unsigned)((const gint*)count)[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(report + 1, tag | (unsigned)((const gint*)count)[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(report + 2, tag | (unsigned)((const gint*)count)[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#endif	// SAI2B_N == 7

int launch_tick_self(const DevParams* d_params, int B, const TickForm& form, bool with_comp, const WorkList& fb, unsigned stamp,
					 hipStream_t stream) {
#if SAI2B_N == 7
	if (form.fast != 1 && form.fast != 2) return 1;
	// [FAST - 1][BAKED]
	static constexpr decltype(&tick_self_kernel<1, false>) kernel[2][2] = {{tick_self_kernel<1, false>, tick_self_kernel<1, true>},
																		   {tick_self_kernel<2, false>, tick_self_kernel<2, true>}};
	hipLaunchKernelGGL(kernel[form.fast == 2][form.baked], dim3((B + 63) / 64), dim3(64), 0, stream, d_params, d_params, with_comp ? 1 : 0,
					   fb.counts, fb.parity);
	if (stamp && fb.report) hipLaunchKernelGGL(worklist_report_kernel, dim3(1), dim3(1), 0, stream, fb.count(), fb.report, stamp);
	return launch_result();
#else
	return 1;  // (never chosen: the SVD-free headline kernels are for 7-joint robots)
#endif
}

}  // namespace sai2b

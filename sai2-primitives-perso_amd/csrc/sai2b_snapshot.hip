// sai2b_snapshot.hip — whole robot states between a context and a snapshot bank (include/sai2b.h "snapshot banks"): save and
// load are one kernel template that differs in direction. No arithmetic: 8-byte blocks move as 8-byte integers and 4-byte
// blocks as 4-byte integers, so every bit pattern (NaN payloads included) survives.
//
// One lane per robot column, one wavefront per workgroup, as everywhere in this library. A lane reads mask[b] and slot[b]
// once; a wavefront without a selected robot leaves after that (the vote is uniform, as in reset_subset_kernel). The lane
// then walks the row table the host uploaded with the bank (sai2b_snapshot_layout.h, each block with its base pointer): the
// kernel reads nothing of DevParams. The table is batch-uniform, so its reads are scalar loads and the walk is uniform.
// The grid's second dimension splits the table's rows into chunks of SNAP_CHUNK_ROWS, so that a save of 65 536 robots is not
// 1 024 wavefronts walking ~1 700 rows one after the other. The context is [row][B], the bank [word][capacity]: with the
// identity slot map a wavefront's 64 lanes touch 512 contiguous bytes on both sides, and a clone reads one bank address
// per row (a broadcast).
//
// Counts (robots moved, slot out of range, slot never saved): chunk 0's wavefronts add theirs to three device words; the last
// of them to arrive (a ticket) writes the three totals, tagged with the call's stamp, to mapped host words (system scope) and
// clears the device words for the next call. No copy follows the launch.
#include <hip/hip_runtime.h>

#include "sai2b_launch.h"

namespace sai2b {

// One lane of every wavefront of chunk 0 comes here once its counts are added. The last to arrive hands the totals to the host:
// three tagged 8-byte words in mapped memory (never a torn set), and the device words are zero again for the next call.
__device__ inline void snapshot_ticket(const SnapArgs& A) {
	__threadfence();
	const int ticket = atomicAdd(A.counts + 3, 1);
	if (ticket != (int)gridDim.x - 1) return;
	__threadfence();
	const unsigned long long tag = (unsigned long long)A.stamp << 32;
	for (int k = 0; k < 3; k++)
		__hip_atomic_store(A.report + k, tag | (unsigned)atomicExch(A.counts + k, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	atomicExch(A.counts + 3, 0);
}

template <bool SAVE>
__global__ __launch_bounds__(64) void snapshot_kernel(const SnapArgs A) {
	const int B = A.B, cap = A.capacity;
	const int b = blockIdx.x * 64 + threadIdx.x;
	const bool in_batch = b < B;
	const int bc = in_batch ? b : B - 1;
	const bool selected = in_batch && (A.mask ? A.mask[bc] != 0 : true);
	const bool first_chunk = blockIdx.y == 0;
	// a load while the state buffer is every robot's cached pose: the flag ends for the batch, so the robots this call leaves alone
	// get their q_pose column from q (chunk 0 does it; a robot that is loaded gets the column from the bank)
	const bool keep_pose = !SAVE && A.keep_pose_q != nullptr;
	if (!__any(selected) && !(first_chunk && keep_pose)) {
		if (first_chunk && threadIdx.x == 0) {	// the ticket is taken by every wavefront of chunk 0
			snapshot_ticket(A);
		}
		return;
	}
	const int slot = selected ? (A.slot ? A.slot[bc] : b) : 0;
	const bool in_range = selected && slot >= 0 && slot < cap;
	const bool saved = in_range && (SAVE || A.valid[slot] != 0);
	const bool moved = saved;
	if (first_chunk) {
		if (SAVE && moved) A.valid[slot] = 1;
		if (keep_pose && in_batch && !moved)
			for (int i = 0; i < A.dof; i++) A.keep_pose_dst[(size_t)i * B + b] = A.keep_pose_q[(size_t)i * B + b];
		const int n_moved = __popcll(__ballot(moved)), n_range = __popcll(__ballot(selected && !in_range)),
				  n_unsaved = __popcll(__ballot(in_range && !saved));
		if (threadIdx.x == 0) {
			if (n_moved) atomicAdd(A.counts + 0, n_moved);
			if (n_range) atomicAdd(A.counts + 1, n_range);
			if (n_unsaved) atomicAdd(A.counts + 2, n_unsaved);
			snapshot_ticket(A);
		}
	}
	if (!moved) return;
	const int r_lo = blockIdx.y * SNAP_CHUNK_ROWS;
	const int r_hi = r_lo + SNAP_CHUNK_ROWS < A.total_rows ? r_lo + SNAP_CHUNK_ROWS : A.total_rows;
#pragma unroll 1
	for (int i = 0; i < A.n_blocks; i++) {
		const SnapDevBlock& blk = A.table[i];
		const int lo = r_lo > blk.first_row ? r_lo - blk.first_row : 0;
		const int hi = r_hi < blk.first_row + blk.rows ? r_hi - blk.first_row : blk.rows;
		if (lo >= hi) continue;
		// a save stores the cached pose whatever buffer holds it at the moment
		char* base = (SAVE && blk.pose && A.pose_src) ? (char*)A.pose_src : (char*)blk.base;
		char* bank = A.bank + (size_t)blk.first_word * (size_t)cap * 4;
		if (blk.elem_bytes == 8) {
			unsigned long long* c = (unsigned long long*)base + b;
			unsigned long long* k = (unsigned long long*)bank + slot;
#pragma unroll 4
			for (int r = lo; r < hi; r++) {
				if (SAVE)
					k[(size_t)r * cap] = c[(size_t)r * B];
				else
					c[(size_t)r * B] = k[(size_t)r * cap];
			}
		} else {
			unsigned* c = (unsigned*)base + b;
			unsigned* k = (unsigned*)bank + slot;
#pragma unroll 4
			for (int r = lo; r < hi; r++) {
				if (SAVE)
					k[(size_t)r * cap] = c[(size_t)r * B];
				else
					c[(size_t)r * B] = k[(size_t)r * cap];
			}
		}
	}
}

int launch_snapshot(const SnapArgs& args, bool save, hipStream_t stream) {
	const int chunks = (args.total_rows + SNAP_CHUNK_ROWS - 1) / SNAP_CHUNK_ROWS;
	const dim3 grid((args.B + 63) / 64, chunks > 0 ? chunks : 1), block(64);
	if (save)
		hipLaunchKernelGGL(snapshot_kernel<true>, grid, block, 0, stream, args);
	else
		hipLaunchKernelGGL(snapshot_kernel<false>, grid, block, 0, stream, args);
	return launch_result();
}

}  // namespace sai2b

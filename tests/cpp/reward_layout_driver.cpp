// reward_layout_driver.cpp — hardware_layout_driver.cpp with the field the reward's accumulators add to a description
// (reward) behind the nine it reads: prints the snapshot row table of csrc/sai2b_snapshot_layout.h. The header alone is
// included: built with plain g++ (-DSAI2B_N=<joints>), no HIP, no GPU.
//
//   reward_layout_driver consts
//       "MAX_TABLE value", "BLOCKS value"
//   reward_layout_driver table  what steps contact joint wrench payload plant_payload hardware hardware_depth reward  [kind k0 otg_mode otg3 popc nprec]...
//       "row <block id> <block name> <task> <rows> <elem bytes> <first word> <first row>" per block, then
//       "words <n> rows <n> fingerprint <hex>"
//   reward_layout_driver diff   <description> -- <description>
//       "same", or "differ <text naming the first differing block>"
// kind: enum sai2b_task_type (1 = JointTask, 2 = MotionForceTask).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sai2b_snapshot_layout.h"

using namespace sai2b;

static bool parse(int argc, char** argv, int& i, SnapDesc& d) {
	std::memset(&d, 0, sizeof(d));
	d.dof = N;
	int* head[10] = {&d.what, &d.steps, &d.contact, &d.joint, &d.wrench, &d.payload, &d.plant_payload, &d.hardware, &d.hardware_depth, &d.reward};
	for (int k = 0; k < 10; k++) {
		if (i >= argc || !std::strcmp(argv[i], "--")) return false;
		*head[k] = std::atoi(argv[i++]);
	}
	while (i < argc && std::strcmp(argv[i], "--")) {
		if (d.n_tasks >= SAI2B_MAX_TASKS || i + 6 > argc) return false;
		SnapTaskDesc& t = d.task[d.n_tasks++];
		int* f[6] = {&t.kind, &t.k0, &t.otg_mode, &t.otg3, &t.popc, &t.nprec};
		for (int k = 0; k < 6; k++) {
			if (!std::strcmp(argv[i], "--")) return false;
			*f[k] = std::atoi(argv[i++]);
		}
	}
	return true;
}

int main(int argc, char** argv) {
	if (argc >= 2 && !std::strcmp(argv[1], "consts")) {
		std::printf("MAX_TABLE %d\nBLOCKS %d\n", SNAP_MAX_ROWS_TABLE, (int)SNAP_BLOCKS);
		return 0;
	}
	if (argc >= 2 && !std::strcmp(argv[1], "table")) {
		SnapDesc d;
		int i = 2;
		if (!parse(argc, argv, i, d) || i != argc) return std::fprintf(stderr, "bad description\n"), 2;
		const SnapLayout L = snapshot_layout(d);
		for (int k = 0; k < L.n; k++) {
			const SnapRow& r = L.row[k];
			std::printf("row %d %s %d %d %d %d %d\n", r.block, SNAP_BLOCK_NAME[r.block], r.task, r.rows, r.elem_bytes, r.first_word, r.first_row);
		}
		std::printf("words %d rows %d fingerprint %016llx\n", L.words, L.rows, L.fingerprint);
		return 0;
	}
	if (argc >= 2 && !std::strcmp(argv[1], "diff")) {
		SnapDesc a, b;
		int i = 2;
		if (!parse(argc, argv, i, a) || i >= argc || std::strcmp(argv[i], "--")) return std::fprintf(stderr, "bad first description\n"), 2;
		i++;
		if (!parse(argc, argv, i, b) || i != argc) return std::fprintf(stderr, "bad second description\n"), 2;
		char msg[160] = "";
		if (snapshot_first_difference(a, b, msg, sizeof(msg)))
			std::printf("differ %s\n", msg);
		else
			std::printf("same\n");
		return 0;
	}
	std::fprintf(stderr, "usage: reward_layout_driver consts | table <description> | diff <description> -- <description>\n");
	return 2;
}

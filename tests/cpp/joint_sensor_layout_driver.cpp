// joint_sensor_layout_driver.cpp — snapshot_layout_driver.cpp with every field of a description, the two the joint sensors
// add (joint_sensor, joint_sensor_depth) last: prints the snapshot row table of csrc/sai2b_snapshot_layout.h. The header alone
// is included: built with plain g++ (-DSAI2B_N=<joints>), no HIP, no GPU.
//
//   joint_sensor_layout_driver consts
//       the row constants of sai2b_params.h for this joint count, one "NAME value" per line
//   joint_sensor_layout_driver table  what steps contact joint wrench payload plant_payload hardware hardware_depth
//       reward reset_sampler env_sampler joint_sensor joint_sensor_depth  [kind k0 otg_mode otg3 popc nprec]...
//       "row <block id> <block name> <task> <rows> <elem bytes> <first word> <first row>" per block, then
//       "words <n> rows <n> fingerprint <hex>"
//   joint_sensor_layout_driver diff   <description> -- <description>
//       "same", or "differ <text naming the first differing block>"
// kind: enum sai2b_task_type (1 = JointTask, 2 = MotionForceTask; `consts` prints them).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sai2b_snapshot_layout.h"

using namespace sai2b;

static bool parse(int argc, char** argv, int& i, SnapDesc& d) {
	std::memset(&d, 0, sizeof(d));
	d.dof = N;
	int* head[14] = {&d.what,	 &d.steps,		  &d.contact, &d.joint,		   &d.wrench,	   &d.payload,		&d.plant_payload,
					 &d.hardware, &d.hardware_depth, &d.reward,  &d.reset_sampler, &d.env_sampler, &d.joint_sensor, &d.joint_sensor_depth};
	for (int k = 0; k < 14; k++) {
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
		std::printf("N %d\nOTG_MD %d\nMFT_GOAL_ROWS %d\nMFT_STATE_ROWS %d\nMFT_ISTATE_ROWS %d\nOTG_ROWS %d\nOTG3_STRIDE %d\nPOPC_RING %d\n", N, OTG_MD,
					MFT_GOAL_ROWS, MFT_STATE_ROWS, MFT_ISTATE_ROWS, OTG_ROWS, OTG3_STRIDE, POPC_RING);
		std::printf("PAYLOAD_ROWS %d\nCONTACT_ROWS %d\nCONTACT_STATUS_ROWS %d\nJOINT_TASK %d\nMOTION_FORCE_TASK %d\nMAX_TASKS %d\nMAX_TABLE %d\nROOM %d\nFULL %d\nBLOCKS_ALL %d\nBLOCKS_EVERY %d\n",
					PAYLOAD_ROWS, CONTACT_ROWS, CONTACT_STATUS_ROWS, (int)SAI2B_JOINT_TASK, (int)SAI2B_MOTION_FORCE_TASK, SAI2B_MAX_TASKS,
					SNAP_MAX_ROWS_TABLE, SNAP_TABLE_ROOM, SNAP_TABLE_FULL, (int)SNAP_BLOCKS_ALL, (int)SNAP_BLOCKS_EVERY);
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
	std::fprintf(stderr, "usage: joint_sensor_layout_driver consts | table <description> | diff <description> -- <description>\n");
	return 2;
}

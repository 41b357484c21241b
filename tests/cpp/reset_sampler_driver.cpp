// reset_sampler_driver.cpp — the host-compilable parts of the episode sampler on a CPU: the draws of csrc/sai2b_reset_draw.h, the
// row layout of csrc/sai2b_reset_sampler_layout.h and the snapshot table of csrc/sai2b_snapshot_layout.h with the field the
// sampler adds to a description. Built with plain g++ (-DSAI2B_N=<joints> -ffp-contract=off), no HIP, no GPU.
//
//   reset_sampler_driver draws <counters.u32> <values.f64> <out.f64>
//       records of 6 words (n, e, call, robot, key0, key1) and 32 doubles (lower 4, upper 4, sigma 4, pos_lower 3, pos_upper 3,
//       theta_max, R 9, half_width 4); per record 24 doubles out: candidate q 4, dq 4, goal offset p 3, goal rotation 9, joint
//       goal offsets 4 (the goal draws use the record's n as the task index)
//   reset_sampler_driver rows <goal_tasks> [kind task_dof]...
//       "goal <task> <first row> <rows>" per task with a drawn goal, then "total <rows>"
//   reset_sampler_driver rowcheck <goal_tasks> <B> <rows.f64> [kind task_dof]...
//       what the host checks of rows [total][B] given as a host array, with joint limits of -3 .. 3 for every joint: "ok", or
//       the message
//   reset_sampler_driver consts | table <description> | diff <description> -- <description>
//       as reward_layout_driver, the description's head with reset_sampler as its 11th field
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sai2b_reset_draw.h"
#include "sai2b_reset_sampler_layout.h"
#include "sai2b_snapshot_layout.h"

using namespace sai2b;

static bool parse(int argc, char** argv, int& i, SnapDesc& d) {
	std::memset(&d, 0, sizeof(d));
	d.dof = N;
	int* head[11] = {&d.what, &d.steps, &d.contact, &d.joint, &d.wrench, &d.payload, &d.plant_payload, &d.hardware, &d.hardware_depth, &d.reward,
					 &d.reset_sampler};
	for (int k = 0; k < 11; k++) {
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

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	std::fseek(f, 0, SEEK_END);
	const long bytes = std::ftell(f);
	std::fseek(f, 0, SEEK_SET);
	v.resize(bytes > 0 ? (size_t)bytes / sizeof(T) : 0);
	const size_t got = v.empty() ? 0 : std::fread(v.data(), sizeof(T), v.size(), f);
	std::fclose(f);
	return got == v.size();
}

static int draws(const char* cpath, const char* vpath, const char* opath) {
	std::vector<unsigned> c;
	std::vector<double> v;
	if (!read_all(cpath, c) || !read_all(vpath, v) || c.size() % 6 || v.size() % 32 || c.size() / 6 != v.size() / 32) return 2;
	const size_t R = c.size() / 6;
	std::vector<double> out(24 * R);
	for (size_t r = 0; r < R; r++) {
		const unsigned n = c[6 * r], e = c[6 * r + 1], call = c[6 * r + 2], robot = c[6 * r + 3], k0 = c[6 * r + 4], k1 = c[6 * r + 5];
		const double* in = &v[32 * r];
		double* o = &out[24 * r];
		rs_candidate4(n, e, call, robot, k0, k1, in, in + 4, o);
		rs_velocity4(e, call, robot, k0, k1, in + 8, o + 4);
		double u[4], w[4], axis[3], D[9];
		rs_uniforms4(n, e, RS_STREAM_GOAL, 0u, robot, k0, k1, u);
		rs_uniforms4(n, e, RS_STREAM_GOAL, 1u, robot, k0, k1, w);
		for (int k = 0; k < 3; k++) o[8 + k] = rs_lerp(in[12 + k], in[15 + k], u[k]);
		rs_axis_rotation(in[18] * u[3], w[0], w[1], axis, D);
		rs_rotate(in + 19, D, o + 11);
		rs_uniforms4(n, e, RS_STREAM_GOAL, call, robot, k0, k1, u);
		for (int k = 0; k < 4; k++) o[20 + k] = rs_joint_offset(in[28 + k], u[k]);
	}
	FILE* f = std::fopen(opath, "wb");
	if (!f) return 2;
	const size_t put = std::fwrite(out.data(), sizeof(double), out.size(), f);
	std::fclose(f);
	return put == out.size() ? 0 : 2;
}

int main(int argc, char** argv) {
	if (argc == 5 && !std::strcmp(argv[1], "draws")) return draws(argv[2], argv[3], argv[4]);
	if (argc >= 3 && !std::strcmp(argv[1], "rows") && (argc - 3) % 2 == 0 && (argc - 3) / 2 <= SAI2B_MAX_TASKS) {
		sai2b_reset_sampler_config cfg;
		std::memset(&cfg, 0, sizeof(cfg));
		cfg.goal_tasks = (unsigned)std::strtoul(argv[2], nullptr, 0);
		std::vector<sai2b_task_config> tasks((argc - 3) / 2);
		for (size_t t = 0; t < tasks.size(); t++) {
			std::memset(&tasks[t], 0, sizeof(sai2b_task_config));
			tasks[t].type = std::atoi(argv[3 + 2 * t]), tasks[t].task_dof = std::atoi(argv[4 + 2 * t]);
		}
		const RsLayout L = rs_layout(cfg, tasks.data(), (int)tasks.size(), N);
		for (size_t t = 0; t < tasks.size(); t++)
			if (L.goal_first[t] >= 0) std::printf("goal %d %d %d\n", (int)t, L.goal_first[t], L.goal_rows[t]);
		std::printf("total %d\n", L.total);
		return 0;
	}
	if (argc >= 5 && !std::strcmp(argv[1], "rowcheck") && (argc - 5) % 2 == 0 && (argc - 5) / 2 <= SAI2B_MAX_TASKS) {
		sai2b_reset_sampler_config cfg;
		std::memset(&cfg, 0, sizeof(cfg));
		cfg.goal_tasks = (unsigned)std::strtoul(argv[2], nullptr, 0);
		const size_t B = (size_t)std::atoi(argv[3]);
		std::vector<sai2b_task_config> tasks((argc - 5) / 2);
		for (size_t t = 0; t < tasks.size(); t++) {
			std::memset(&tasks[t], 0, sizeof(sai2b_task_config));
			tasks[t].type = std::atoi(argv[5 + 2 * t]), tasks[t].task_dof = std::atoi(argv[6 + 2 * t]);
		}
		const RsLayout L = rs_layout(cfg, tasks.data(), (int)tasks.size(), N);
		std::vector<double> rows;
		if (!read_all(argv[4], rows) || rows.size() != (size_t)L.total * B) return std::fprintf(stderr, "rows must be [%d][B]\n", L.total), 2;
		double q_min[N], q_max[N];
		for (int i = 0; i < N; i++) q_min[i] = -3.0, q_max[i] = 3.0;
		const std::string err = rs_rows_error(L, tasks.data(), (int)tasks.size(), N, q_min, q_max, rows.data(), B);
		std::printf("%s\n", err.empty() ? "ok" : err.c_str());
		return 0;
	}
	if (argc >= 2 && !std::strcmp(argv[1], "consts")) {
		std::printf("MAX_TABLE %d\nCAPACITY %d\nBLOCKS %d\n", SNAP_MAX_ROWS_TABLE, SNAP_TABLE_CAPACITY, (int)SNAP_BLOCKS);
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
	std::fprintf(stderr, "usage: reset_sampler_driver draws <counters> <values> <out> | rows <goal_tasks> [kind dof]... | consts | table .. | diff ..\n");
	return 2;
}

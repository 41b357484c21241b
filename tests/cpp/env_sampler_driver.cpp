// env_sampler_driver.cpp — the host-compilable parts of the environment sampler on a CPU: the draws of csrc/sai2b_env_draw.h, the
// sample-row layout and the host checks of csrc/sai2b_env_sampler_layout.h and the snapshot table of csrc/sai2b_snapshot_layout.h
// with the field the sampler adds to a description. Built with plain g++ (-DSAI2B_N=<joints> -ffp-contract=off), no HIP, no GPU.
//
//   env_sampler_driver draws <counters.u32> <values.f64> <out.f64>
//       records of 4 words (c, robot, key0, key1) and IN doubles:
//         15 ranges of (lower, upper, log_uniform) in the order payload_mass, contact_height, contact stiffness / damping /
//         friction, armature, damping, friction, torque_limit, lag, gain, torque_noise, sensor_noise, push_force, push_moment;
//         payload_com_half 3, contact_tilt_max, sensor_bias_half 6; delay_lower, delay_upper, steps_lower, steps_upper;
//         nominal payload 10, contact 9, joint chunk 4, hardware chunk 4, sensor 12; joint p, joint j, hardware p, hardware j
//       per record OUT doubles: payload sample 4, rows 10; contact rows 9, sample 8; joint rows 4, sample 4; hardware rows 4,
//       sample 4, clipped bits; delay; sensor rows 12, sample 7; push rows 7, sample 9
//   env_sampler_driver layout <groups>
//       "group <bit> <first row> <rows>" per configured group, then "total <rows>"
//   env_sampler_driver consts | table <description> | diff <description> -- <description>
//       as reset_sampler_driver, the description's head with env_sampler as its 12th field
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sai2b_env_draw.h"
#include "sai2b_env_sampler_layout.h"
#include "sai2b_snapshot_layout.h"

using namespace sai2b;

constexpr int IN = 102, OUT = 84;

static bool parse(int argc, char** argv, int& i, SnapDesc& d) {
	std::memset(&d, 0, sizeof(d));
	d.dof = N;
	int* head[12] = {&d.what,	 &d.steps,	  &d.contact,		 &d.joint,	&d.wrench,		  &d.payload, &d.plant_payload,
					 &d.hardware, &d.hardware_depth, &d.reward, &d.reset_sampler, &d.env_sampler};
	for (int k = 0; k < 12; k++) {
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

// the first 59 doubles of a record as a configuration
static sai2b_env_sampler_config config_of(const double* in) {
	sai2b_env_sampler_config c;
	env_default_config(&c);
	sai2b_env_range* const ranges[15] = {&c.payload_mass_scale,	   &c.contact_height, &c.contact_stiffness_scale, &c.contact_damping_scale,
										 &c.contact_friction_scale, &c.armature_scale, &c.damping_scale,		   &c.friction_scale,
										 &c.torque_limit_scale,	   &c.lag_scale,	  &c.gain_scale,			   &c.torque_noise_scale,
										 &c.sensor_noise_scale,	   &c.push_force,	  &c.push_moment};
	for (int k = 0; k < 15; k++) ranges[k]->lower = in[3 * k], ranges[k]->upper = in[3 * k + 1], ranges[k]->log_uniform = (int)in[3 * k + 2];
	for (int k = 0; k < 3; k++) c.payload_com_half[k] = in[45 + k];
	c.contact_tilt_max = in[48];
	for (int k = 0; k < 6; k++) c.sensor_bias_half[k] = in[49 + k];
	c.delay_lower = (int)in[55], c.delay_upper = (int)in[56], c.push_steps_lower = (int)in[57], c.push_steps_upper = (int)in[58];
	return c;
}

static int draws(const char* cpath, const char* vpath, const char* opath) {
	std::vector<unsigned> c;
	std::vector<double> v;
	if (!read_all(cpath, c) || !read_all(vpath, v) || c.size() % 4 || v.size() % IN || c.size() / 4 != v.size() / IN) return 2;
	const size_t R = c.size() / 4;
	std::vector<double> out(OUT * R);
	for (size_t r = 0; r < R; r++) {
		const unsigned cnt = c[4 * r], robot = c[4 * r + 1], k0 = c[4 * r + 2], k1 = c[4 * r + 3];
		const double* in = &v[IN * r];
		double* o = &out[OUT * r];
		const EnvDraw D = env_draw_params(config_of(in));
		const double* nom = in + 59;
		const int jp = (int)in[98], jj = (int)in[99], hp = (int)in[100], hj = (int)in[101];
		env_payload_sample(D, cnt, robot, k0, k1, o);
		env_payload_apply(o, nom, o + 4);
		env_contact(D, cnt, robot, k0, k1, nom + 10, o + 14, o + 23);
		env_joint4(D, jp, jj, cnt, robot, k0, k1, nom + 19, o + 31, o + 35);
		o[47] = (double)env_hardware4(D, hp, hj, cnt, robot, k0, k1, nom + 23, o + 39, o + 43);
		o[48] = env_delay(D, cnt, robot, k0, k1);
		env_sensor(D, cnt, robot, k0, k1, nom + 27, o + 49, o + 61);
		env_push(D, cnt, robot, k0, k1, o + 68, o + 75);
	}
	FILE* f = std::fopen(opath, "wb");
	if (!f) return 2;
	const size_t put = std::fwrite(out.data(), sizeof(double), out.size(), f);
	std::fclose(f);
	return put == out.size() ? 0 : 2;
}

int main(int argc, char** argv) {
	if (argc == 5 && !std::strcmp(argv[1], "draws")) return draws(argv[2], argv[3], argv[4]);
	if (argc == 3 && !std::strcmp(argv[1], "layout")) {
		const unsigned groups = (unsigned)std::strtoul(argv[2], nullptr, 0) & ENV_ALL_GROUPS;
		const EnvLayout L = env_layout(groups, N);
		for (int g = 0; g < ENV_GROUPS; g++)
			if (L.first[g] >= 0) std::printf("group %d %d %d\n", 1 << g, L.first[g], L.rows[g]);
		std::printf("total %d\n", L.total);
		return 0;
	}
	if (argc >= 2 && !std::strcmp(argv[1], "consts")) {
		std::printf("MAX_TABLE %d\nCAPACITY %d\nROOM %d\nBLOCKS %d\nBLOCKS_ALL %d\n", SNAP_MAX_ROWS_TABLE, SNAP_TABLE_CAPACITY, SNAP_TABLE_ROOM,
					(int)SNAP_BLOCKS, (int)SNAP_BLOCKS_ALL);
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
	std::fprintf(stderr, "usage: env_sampler_driver draws <counters> <values> <out> | layout <groups> | consts | table .. | diff ..\n");
	return 2;
}

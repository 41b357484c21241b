// ik_driver.cpp — the inverse-kinematics law (csrc/sai2b_ik_law.h) on a CPU: the same code ik_kernel runs per lane, here per
// record with stride 1. The header alone is included: built with plain g++, no HIP, no GPU.
//
//   ik_driver law   <ints.i32> <values.f64> <out.f64>
//   ik_driver seeds <ints.i32> <values.f64> <out.f64>
//       records of INTS ints (dof, link, max_iterations, restarts, use_limits, has_rest, key0, key1, first_robot, draw_id, robot,
//       jtype 8) and IN doubles, every array in a slot sized for 8 joints and packed from its start for fewer: E 72, xyz 24, lo 8,
//       hi 8, frame_pos 3, frame_rot 9, w2 6, sel 6, tol_pos, tol_rot, mu0, mu_min, mu_max, mu_down, mu_up, step_max, rest_weight,
//       goal 12, rest 8, seed 8.
//       law: per record OUT doubles: q_out 8, status 5, flags 1 (q_out and status keep -7.25 where the law writes nothing).
//       seeds: per record OUT doubles: the seed of start `restarts` (>= 1) in q_out's slot, the rest zero.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sai2b_ik_law.h"

using namespace sai2b;

constexpr int INTS = 11 + 8, IN = 72 + 24 + 16 + 12 + 12 + 9 + 12 + 16, OUT = 8 + 5 + 1;
constexpr double SENTINEL = -7.25;

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

template <int DOF>
static void one(bool seeds, const int* c, const double* in, double* o) {
	IkLaw<DOF> G;
	const double *E = in, *xyz = in + 72, *lo = in + 96, *hi = in + 104, *fp = in + 112, *fr = in + 115, *w2 = in + 124, *sel = in + 130, *s = in + 136,
				 *goal = in + 145, *rest = in + 157, *seed = in + 165;
	for (int i = 0; i < DOF; i++) {
		for (int a = 0; a < 9; a++) G.E[i][a] = E[9 * i + a];
		for (int a = 0; a < 3; a++) G.xyz[i][a] = xyz[3 * i + a];
		G.jtype[i] = c[11 + i];
		G.lo[i] = lo[i], G.hi[i] = hi[i];
	}
	G.link = c[1], G.max_iterations = c[2], G.restarts = c[3], G.use_limits = c[4];
	for (int a = 0; a < 3; a++) G.frame_pos[a] = fp[a];
	for (int a = 0; a < 9; a++) G.frame_rot[a] = fr[a];
	for (int a = 0; a < 6; a++) G.w2[a] = w2[a], G.sel[a] = sel[a];
	G.tol_pos = s[0], G.tol_rot = s[1], G.mu0 = s[2], G.mu_min = s[3], G.mu_max = s[4], G.mu_down = s[5], G.mu_up = s[6], G.step_max = s[7];
	G.rest_weight = s[8];
	G.key0 = (unsigned)c[6], G.key1 = (unsigned)c[7], G.first_robot = (unsigned)c[8], G.draw_id = (unsigned)c[9];
	if (seeds) {
		double q[DOF];
		ik_restart_seed<DOF>(G, (unsigned)c[3], (unsigned)c[10], q);
		for (int i = 0; i < DOF; i++) o[i] = q[i];
		return;
	}
	double q[DOF], status[IK_STATUS_ROWS];
	for (int i = 0; i < DOF; i++) q[i] = SENTINEL;
	for (int i = 0; i < IK_STATUS_ROWS; i++) status[i] = SENTINEL;
	const int flags = ik_law<DOF>(G, true, goal, c[5] ? rest : nullptr, seed, 1, (unsigned)c[10], q, status);
	for (int i = 0; i < DOF; i++) o[i] = q[i];
	for (int i = 0; i < IK_STATUS_ROWS; i++) o[8 + i] = status[i];
	o[13] = (double)flags;
}

int main(int argc, char** argv) {
	if (argc != 5 || (std::strcmp(argv[1], "law") && std::strcmp(argv[1], "seeds"))) {
		std::fprintf(stderr, "usage: ik_driver law|seeds <ints> <values> <out>\n");
		return 2;
	}
	const bool seeds = !std::strcmp(argv[1], "seeds");
	std::vector<int> c;
	std::vector<double> v;
	if (!read_all(argv[2], c) || !read_all(argv[3], v) || c.size() % INTS || v.size() % IN || c.size() / INTS != v.size() / IN) return 2;
	const size_t R = c.size() / INTS;
	std::vector<double> out(OUT * R, 0.0);
	for (size_t r = 0; r < R; r++) {
		const int* k = &c[INTS * r];
		if (k[1] < 0 || k[1] >= k[0] || k[2] < 1 || k[2] > IK_MAX_ITERATIONS || k[3] < 0 || k[3] > IK_MAX_RESTARTS) return 2;
		switch (k[0]) {
			case 4: one<4>(seeds, k, &v[IN * r], &out[OUT * r]); break;
			case 6: one<6>(seeds, k, &v[IN * r], &out[OUT * r]); break;
			case 7: one<7>(seeds, k, &v[IN * r], &out[OUT * r]); break;
			case 8: one<8>(seeds, k, &v[IN * r], &out[OUT * r]); break;
			default: return 2;
		}
	}
	FILE* f = std::fopen(argv[4], "wb");
	if (!f) return 2;
	const size_t put = std::fwrite(out.data(), sizeof(double), out.size(), f);
	std::fclose(f);
	return put == out.size() ? 0 : 2;
}

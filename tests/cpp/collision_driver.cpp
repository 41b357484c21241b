// collision_driver.cpp — the collision-proximity law (csrc/sai2b_collision_law.h) on a CPU: the same code collision_kernel runs
// per lane, here per record with stride 1. The header alone is included: built with plain g++, no HIP, no GPU.
//
//   collision_driver law <ints.i32> <values.f64> <out.f64>
//       records of INTS ints (dof, n_spheres, n_planes, n_obstacles, env_mask, pair_mask 16, link 16, jtype 8) and IN doubles, every
//       array in a slot sized for 8 joints, 16 spheres, 2 planes and 4 obstacles and packed from its start for fewer: E 72, xyz 24,
//       centre 48, radius 16, margin 3, q 8, env 28;
//       per record OUT doubles: distance 3, index 3, normal 9, gradient 3 x 8 (a category's dof entries from the start of its
//       slot), centres 48, flags 1. Every block is computed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sai2b_collision_law.h"

using namespace sai2b;

constexpr int INTS = 5 + 16 + 16 + 8, IN = 72 + 24 + 48 + 16 + 3 + 8 + 28, OUT = 3 + 3 + 9 + 24 + 48 + 1;

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
static void one(const int* c, const double* in, double* o) {
	ColLaw<DOF> G;
	const double *E = in, *xyz = in + 72, *centre = in + 96, *radius = in + 144, *margin = in + 160, *q = in + 163, *env = in + 171;
	for (int i = 0; i < DOF; i++) {
		for (int a = 0; a < 9; a++) G.E[i][a] = E[9 * i + a];
		for (int a = 0; a < 3; a++) G.xyz[i][a] = xyz[3 * i + a];
		G.jtype[i] = c[37 + i];
	}
	G.n_spheres = c[1], G.n_planes = c[2], G.n_obstacles = c[3], G.blocks = COL_ALL_BLOCKS;
	G.env_mask = (unsigned)c[4];
	for (int k = 0; k < COL_MAX_SPHERES; k++) {
		G.pair_mask[k] = (unsigned)c[5 + k];
		G.link[k] = c[21 + k];
		for (int a = 0; a < 3; a++) G.centre[k][a] = centre[3 * k + a];
		G.radius[k] = radius[k];
	}
	for (int a = 0; a < COL_CATEGORIES; a++) G.margin[a] = margin[a];
	const int rows = col_layout(G.blocks, DOF, G.n_spheres, G.row);
	std::vector<double> out(rows, 0.0);
	const int flags = collision_law<DOF>(G, q, env, 1, out.data());
	std::memcpy(o, &out[G.row[0]], 3 * sizeof(double));
	std::memcpy(o + 3, &out[G.row[1]], 3 * sizeof(double));
	std::memcpy(o + 6, &out[G.row[2]], 9 * sizeof(double));
	for (int cat = 0; cat < COL_CATEGORIES; cat++) std::memcpy(o + 15 + 8 * cat, &out[G.row[3] + DOF * cat], DOF * sizeof(double));
	std::memcpy(o + 39, &out[G.row[4]], 3 * G.n_spheres * sizeof(double));
	o[87] = (double)flags;
}

int main(int argc, char** argv) {
	if (argc != 5 || std::strcmp(argv[1], "law")) {
		std::fprintf(stderr, "usage: collision_driver law <ints> <values> <out>\n");
		return 2;
	}
	std::vector<int> c;
	std::vector<double> v;
	if (!read_all(argv[2], c) || !read_all(argv[3], v) || c.size() % INTS || v.size() % IN || c.size() / INTS != v.size() / IN) return 2;
	const size_t R = c.size() / INTS;
	std::vector<double> out(OUT * R, 0.0);
	for (size_t r = 0; r < R; r++) {
		const int* k = &c[INTS * r];
		if (k[1] < 1 || k[1] > COL_MAX_SPHERES || k[2] < 0 || k[2] > COL_MAX_PLANES || k[3] < 0 || k[3] > COL_MAX_OBSTACLES) return 2;
		switch (k[0]) {
			case 4: one<4>(k, &v[IN * r], &out[OUT * r]); break;
			case 6: one<6>(k, &v[IN * r], &out[OUT * r]); break;
			case 7: one<7>(k, &v[IN * r], &out[OUT * r]); break;
			case 8: one<8>(k, &v[IN * r], &out[OUT * r]); break;
			default: return 2;
		}
	}
	FILE* f = std::fopen(argv[4], "wb");
	if (!f) return 2;
	const size_t put = std::fwrite(out.data(), sizeof(double), out.size(), f);
	std::fclose(f);
	return put == out.size() ? 0 : 2;
}

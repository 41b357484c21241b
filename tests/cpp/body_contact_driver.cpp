// body_contact_driver.cpp — the whole-arm contact law (csrc/sai2b_body_contact_law.h) on a CPU: the same code sim_body_kernel runs
// per lane, here per record with stride 1 and the kinematics of bc_host_kinematics. The header alone is included: built with plain
// g++, no HIP, no GPU.
//
//   body_contact_driver law <ints.i32> <values.f64> <out.f64>
//       records of INTS ints (dof, n_spheres, n_planes, n_obstacles, env_mask, categories, pair_mask 16, link 16, jtype 8) and IN
//       doubles, every array in a slot sized for 8 joints, 16 spheres, 2 planes and 4 obstacles and packed from its start for
//       fewer: E 72, xyz 24, centre 48, radius 16, v_eps 1, rows (k, d, mu) 3, q 8, dq 8, env 28;
//       per record OUT doubles: depth 3, index 3, sum of f_n 3, tb 8 (the status of the law), then tb of the call without the
//       status 8 (the form the substep loop runs).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sai2b_body_contact_law.h"

using namespace sai2b;

constexpr int INTS = 6 + 16 + 16 + 8, IN = 72 + 24 + 48 + 16 + 1 + 3 + 8 + 8 + 28, OUT = 9 + 8 + 8;

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
static void one(const int* c, const double* in, double* out) {
	const double *E = in, *xyz = in + 72, *centre = in + 96, *radius = in + 144, *rows = in + 161, *q = in + 164, *dq = in + 172, *env = in + 180;
	BcGeom G;
	G.n_spheres = c[1], G.n_planes = c[2], G.n_obstacles = c[3], G.env_mask = (unsigned)c[4], G.categories = c[5];
	G.v_eps = in[160];
	for (int a = 0; a < COL_MAX_SPHERES; a++) {
		G.partner[a] = (unsigned)c[6 + a];
		for (int b = 0; b < a; b++) G.partner[a] |= (((unsigned)c[6 + b] >> a) & 1u) << b;
		G.link[a] = c[22 + a];
		for (int k = 0; k < 3; k++) G.centre[a][k] = centre[3 * a + k];
		G.radius[a] = radius[a];
	}
	const int* jtype = c + 38;
	double z[DOF][3], o[DOF][3], xs[3 * COL_MAX_SPHERES], tw[6 * DOF], tb[DOF], tb2[DOF];
	const double origin[3] = {0, 0, 0};
	bc_host_kinematics<DOF>(G, E, xyz, jtype, q, dq, z, o, xs, tw);
	BcStatus st;
	body_contact_law<DOF, true>(G, xs, tw, 1, z, o, jtype, origin, env, 1, rows[0], rows[1], rows[2], tb, &st);
	body_contact_law<DOF, false>(G, xs, tw, 1, z, o, jtype, origin, env, 1, rows[0], rows[1], rows[2], tb2, nullptr);
	for (int k = 0; k < 3; k++) out[k] = st.depth[k], out[3 + k] = (double)st.index[k], out[6 + k] = st.fsum[k];
	for (int m = 0; m < DOF; m++) out[9 + m] = tb[m], out[17 + m] = tb2[m];
}

int main(int argc, char** argv) {
	if (argc != 5 || std::strcmp(argv[1], "law")) {
		std::fprintf(stderr, "usage: body_contact_driver law <ints> <values> <out>\n");
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
		for (int a = 0; a < COL_MAX_SPHERES; a++)
			if (k[22 + a] < -1 || k[22 + a] >= k[0]) return 2;
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

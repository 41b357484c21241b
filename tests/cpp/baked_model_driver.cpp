// baked_model_driver.cpp — host run of the Panda's written-out model functions (csrc/sai2b_baked_panda_model.h, generated)
// next to the generic formulas of csrc/sai2b_device.hpp restated here on the same constants (csrc/sai2b_baked_panda.h).
//
//   baked_model_driver <file>
// <file>: first line "link fx fy fz pl_link" (task link and control point in it; link of the payload or -1), then one line of
// 7 joint angles per pose. Per pose two lines go to stdout, "S" (written out) and "G" (generic), each holding as hex floats
// x 3, R 9 (frame of `link`), J 42, M 49, g 7, and with a payload M 49 and g 7 again for the payload forms.
// Built by tests/test_baked_model_structure.py with g++, once more with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sai2b_baked_panda.h"
#include "sai2b_baked_panda_model.h"

namespace {
constexpr int N = 7;
using MD = sai2b::PandaBaked;
struct Frames {
	double R[N][9], p[N][3];
};
struct Payload {
	int link;
	double m, c[3], I[6];
};
struct PayloadTerms {
	double m, h[3], IO[6];
};

void mm3(const double* A, const double* B, double* C) {
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) {
			double s = 0;
			for (int l = 0; l < 3; l++) s = std::fma(A[i * 3 + l], B[l * 3 + j], s);
			C[i * 3 + j] = s;
		}
}
void cross3(const double* a, const double* b, double* c) {
	c[0] = a[1] * b[2] - a[2] * b[1];
	c[1] = a[2] * b[0] - a[0] * b[2];
	c[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- the generic functions (every joint revolute, as PandaBaked::jtype says)
void fk(const double* sn, const double* cs, Frames& F) {
	double Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pp[3] = {0, 0, 0};
	for (int i = 0; i < N; i++) {
		double RE[9];
		if (i == 0) {
			for (int k = 0; k < 3; k++) F.p[0][k] = MD::xyz[0][k];
			for (int k = 0; k < 9; k++) RE[k] = MD::E[0][k];
		} else {
			for (int k = 0; k < 3; k++)
				F.p[i][k] = std::fma(Rp[3 * k], MD::xyz[i][0], std::fma(Rp[3 * k + 1], MD::xyz[i][1], std::fma(Rp[3 * k + 2], MD::xyz[i][2], pp[k])));
			mm3(Rp, MD::E[i], RE);
		}
		const double s = sn[i], c = cs[i];
		for (int k = 0; k < 3; k++) {
			F.R[i][3 * k + 0] = std::fma(c, RE[3 * k], s * RE[3 * k + 1]);
			F.R[i][3 * k + 1] = std::fma(c, RE[3 * k + 1], -s * RE[3 * k]);
			F.R[i][3 * k + 2] = RE[3 * k + 2];
		}
		for (int k = 0; k < 9; k++) Rp[k] = F.R[i][k];
		for (int k = 0; k < 3; k++) pp[k] = F.p[i][k];
	}
}
void jacobian(const Frames& F, int link, const double* x, double* J) {
	for (int i = 0; i < N; i++) {
		const double z[3] = {F.R[i][2], F.R[i][5], F.R[i][8]};
		const double d[3] = {x[0] - F.p[i][0], x[1] - F.p[i][1], x[2] - F.p[i][2]};
		double v[3];
		cross3(z, d, v);
		for (int k = 0; k < 3; k++) {
			J[k * N + i] = i <= link ? v[k] : 0.0;
			J[(3 + k) * N + i] = i <= link ? z[k] : 0.0;
		}
	}
}
void payload_terms(const Payload& pl, const Frames& F, PayloadTerms& t) {
	t.m = 0;
	for (double& v : t.h) v = 0;
	for (double& v : t.IO) v = 0;
	const int at = pl.link < 0 ? N - 1 : pl.link;  // (the generic form computes them for the last link, and adds them nowhere)
	const double *R = F.R[at], *p = F.p[at];
	double c[3], Il[9] = {pl.I[0], pl.I[3], pl.I[4], pl.I[3], pl.I[1], pl.I[5], pl.I[4], pl.I[5], pl.I[2]}, T[9];
	for (int a = 0; a < 3; a++) c[a] = std::fma(R[3 * a], pl.c[0], std::fma(R[3 * a + 1], pl.c[1], std::fma(R[3 * a + 2], pl.c[2], p[a])));
	mm3(R, Il, T);
	const double c2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
	const int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
	for (int e = 0; e < 6; e++) {
		double s = 0;
		for (int l = 0; l < 3; l++) s = std::fma(T[3 * ia[e] + l], R[3 * ib[e] + l], s);
		t.IO[e] += s + pl.m * ((ia[e] == ib[e] ? c2 : 0.0) - c[ia[e]] * c[ib[e]]);
	}
	t.m += pl.m;
	for (int a = 0; a < 3; a++) t.h[a] = std::fma(pl.m, c[a], t.h[a]);
}
void link_com(const Frames& F, int k, double* c) {
	const double* R = F.R[k];
	for (int a = 0; a < 3; a++)
		c[a] = std::fma(R[3 * a], MD::com[k][0], std::fma(R[3 * a + 1], MD::com[k][1], std::fma(R[3 * a + 2], MD::com[k][2], F.p[k][a])));
}
void mass_matrix(const Frames& F, double* M, const Payload* pl) {
	double z[N][3], v[N][3];
	for (int i = 0; i < N; i++) {
		const double ax[3] = {F.R[i][2], F.R[i][5], F.R[i][8]};
		cross3(F.p[i], ax, v[i]);
		for (int k = 0; k < 3; k++) z[i][k] = ax[k];
	}
	double mt = 0, h[3] = {0, 0, 0}, IO[6] = {0, 0, 0, 0, 0, 0};
	PayloadTerms pt;
	if (pl) payload_terms(*pl, F, pt);
	for (int k = N - 1; k >= 0; k--) {
		const double* R = F.R[k];
		double c[3];
		link_com(F, k, c);
		const double* li = MD::inertia[k];
		double Il[9] = {li[0], li[3], li[4], li[3], li[1], li[5], li[4], li[5], li[2]}, T[9];
		mm3(R, Il, T);
		const double m = MD::mass[k];
		const double c2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
		const int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
		for (int e = 0; e < 6; e++) {
			double s = 0;
			for (int l = 0; l < 3; l++) s = std::fma(T[3 * ia[e] + l], R[3 * ib[e] + l], s);
			IO[e] += s + m * ((ia[e] == ib[e] ? c2 : 0.0) - c[ia[e]] * c[ib[e]]);
		}
		mt += m;
		for (int a = 0; a < 3; a++) h[a] = std::fma(m, c[a], h[a]);
		if (pl) {
			const bool here = pl->link == k;
			mt += here ? pt.m : 0.0;
			for (int a = 0; a < 3; a++) h[a] += here ? pt.h[a] : 0.0;
			for (int e = 0; e < 6; e++) IO[e] += here ? pt.IO[e] : 0.0;
		}
		double n[3], f[3], hv[3], hz[3];
		cross3(h, v[k], hv);
		cross3(h, z[k], hz);
		n[0] = IO[0] * z[k][0] + IO[3] * z[k][1] + IO[4] * z[k][2] + hv[0];
		n[1] = IO[3] * z[k][0] + IO[1] * z[k][1] + IO[5] * z[k][2] + hv[1];
		n[2] = IO[4] * z[k][0] + IO[5] * z[k][1] + IO[2] * z[k][2] + hv[2];
		for (int a = 0; a < 3; a++) f[a] = mt * v[k][a] - hz[a];
		for (int j = 0; j <= k; j++) {
			const double s = z[j][0] * n[0] + z[j][1] * n[1] + z[j][2] * n[2] + v[j][0] * f[0] + v[j][1] * f[1] + v[j][2] * f[2];
			M[k * N + j] = s;
			M[j * N + k] = s;
		}
	}
}
void gravity_vector(const Frames& F, double* g, const Payload* pl) {
	double mt = 0, h[3] = {0, 0, 0};
	PayloadTerms pt;
	if (pl) payload_terms(*pl, F, pt);
	for (int k = N - 1; k >= 0; k--) {
		const double* R = F.R[k];
		double c[3];
		link_com(F, k, c);
		mt += MD::mass[k];
		for (int a = 0; a < 3; a++) h[a] = std::fma(MD::mass[k], c[a], h[a]);
		if (pl) {
			const bool here = pl->link == k;
			mt += here ? pt.m : 0.0;
			for (int a = 0; a < 3; a++) h[a] += here ? pt.h[a] : 0.0;
		}
		const double d[3] = {h[0] - mt * F.p[k][0], h[1] - mt * F.p[k][1], h[2] - mt * F.p[k][2]};
		const double zk[3] = {R[2], R[5], R[8]};
		double x[3];
		cross3(zk, d, x);
		g[k] = -(x[0] * MD::gravity[0] + x[1] * MD::gravity[1] + x[2] * MD::gravity[2]);
	}
}

void put(const double* v, int n) {
	for (int i = 0; i < n; i++) std::printf(" %a", v[i]);
}
// the pose of the control point, then everything else, from one set of frames
void report(char tag, bool written_out, const double* sn, const double* cs, int link, const double* fpos, const Payload* pl) {
	Frames F;
	if (written_out)
		sai2b::panda_fk(sn, cs, F);
	else
		fk(sn, cs, F);
	double x[3], J[6 * N], M[N * N], g[N];
	for (int k = 0; k < 3; k++)
		x[k] = std::fma(F.R[link][3 * k], fpos[0], std::fma(F.R[link][3 * k + 1], fpos[1], std::fma(F.R[link][3 * k + 2], fpos[2], F.p[link][k])));
	if (written_out) {
		sai2b::panda_jacobian(F, link, x, J);
		sai2b::panda_mass_matrix(F, M);
		sai2b::panda_gravity_vector(F, g);
	} else {
		jacobian(F, link, x, J);
		mass_matrix(F, M, nullptr);
		gravity_vector(F, g, nullptr);
	}
	std::printf("%c", tag);
	put(x, 3), put(F.R[link], 9), put(J, 6 * N), put(M, N * N), put(g, N);
	if (pl) {
		if (written_out) {
			PayloadTerms pt;
			payload_terms(*pl, F, pt);
			sai2b::panda_mass_matrix_payload(F, pl->link, pt, M);
			sai2b::panda_gravity_vector_payload(F, pl->link, pt, g);
		} else {
			mass_matrix(F, M, pl);
			gravity_vector(F, g, pl);
		}
		put(M, N * N), put(g, N);
	}
	std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
	if (argc != 2) return 2;
	std::FILE* f = std::fopen(argv[1], "r");
	if (!f) return 2;
	int link, pl_link;
	double fpos[3];
	if (std::fscanf(f, "%d %lf %lf %lf %d", &link, &fpos[0], &fpos[1], &fpos[2], &pl_link) != 5 || link < 0 || link >= N || pl_link >= N) return 2;
	// a body with products of inertia, off the link's axes
	const Payload pl{pl_link, 1.7, {0.03, -0.05, 0.08}, {0.02, 0.03, 0.025, 0.004, -0.003, 0.002}};
	std::vector<double> q(N);
	for (;;) {
		int got = 0;
		for (int i = 0; i < N; i++) got += std::fscanf(f, "%lf", &q[i]) == 1;
		if (got != N) break;
		double sn[N], cs[N];
		for (int i = 0; i < N; i++) sn[i] = std::sin(q[i]), cs[i] = std::cos(q[i]);
		report('S', true, sn, cs, link, fpos, pl_link >= 0 ? &pl : nullptr);
		report('G', false, sn, cs, link, fpos, pl_link >= 0 ? &pl : nullptr);
	}
	std::fclose(f);
	return 0;
}

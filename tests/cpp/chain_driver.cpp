// chain_driver.cpp — runs csrc/sai2b_chain.h (the two-level fast tick behind the model phase: one whitened chain,
// Householder QR, nullspace pair) on the CPU, next to the algorithm it replaced (two chains on Mb and M, Gram matrix +
// Cholesky, pivot search and one re-orthogonalisation pass), written out here as it stood. tests/test_chain_host.py
// feeds the cases and compares both with a 40-digit evaluation.
//   stdin, per case:  J (6 x 7 row-major) M (7 x 7) Fu (6) Ff (6) f (7) ddq (7) mft_decoupling jt_decoupling thr with_comp
//   stdout, per case: "new" tau_mft a bb tau (4 x 7), then "old" the same
// Decoupling: 0 full, 1 bounded inertia, 2 impedance (include/sai2b.h).
#include <cmath>
#include <cstdio>

#include "sai2b_chain.h"

namespace {
constexpr int N = 7;
using sai2b::chain::real;

struct Law {
	const real *f, *ddq;
	int prefetched = 0;
	void prefetch() { prefetched++; }
	void prefetch_q() { prefetched += 10; }
	void project(const real* a, real& af, real& aacc) {
		for (int i = 0; i < N; i++) {
			af = std::fma(a[i], f[i], af);
			aacc = std::fma(a[i], ddq[i], aacc);
		}
	}
};

// ---- the previous algorithm
template <int n>
void chol(const real* A, real* L, real* dinv) {
	for (int j = 0; j < n; j++) {
		real s = A[j * n + j];
		for (int k = 0; k < j; k++) s = std::fma(-L[j * n + k], L[j * n + k], s);
		real r = 1.0 / std::sqrt(s);
		dinv[j] = r;
		L[j * n + j] = s * r;
		for (int i = j + 1; i < n; i++) {
			real t = A[i * n + j];
			for (int k = 0; k < j; k++) t = std::fma(-L[i * n + k], L[j * n + k], t);
			L[i * n + j] = t * r;
		}
	}
}
template <int n>
void solve_lower(const real* L, const real* dinv, real* x) {
	for (int i = 0; i < n; i++) {
		real t = x[i];
		for (int k = 0; k < i; k++) t = std::fma(-L[i * n + k], x[k], t);
		x[i] = t * dinv[i];
	}
}
template <int n>
void solve_lower_t(const real* L, const real* dinv, real* x) {
	for (int i = n - 1; i >= 0; i--) {
		real t = x[i];
		for (int k = i + 1; k < n; k++) t = std::fma(-L[k * n + i], x[k], t);
		x[i] = t * dinv[i];
	}
}
void whitened(const real* L, const real* dL, const real* J, real* Y, real* A, real* LA, real* dA) {
	for (int c = 0; c < 6; c++) {
		real col[N];
		for (int i = 0; i < N; i++) col[i] = J[c * N + i];
		solve_lower<N>(L, dL, col);
		for (int i = 0; i < N; i++) Y[i * 6 + c] = col[i];
	}
	for (int i = 0; i < 6; i++)
		for (int j = 0; j <= i; j++) {
			real s = 0;
			for (int l = 0; l < N; l++) s = std::fma(Y[l * 6 + i], Y[l * 6 + j], s);
			A[i * 6 + j] = A[j * 6 + i] = s;
		}
	chol<6>(A, LA, dA);
}
void old_tick(const real* J, const real* M, const real* Fu, const real* Ff, int mft_dec, int jt_dec, real thr, bool with_comp,
			  Law& jt, real* tau, sai2b::chain::Probe& pr) {
	const bool mft_bie = mft_dec == 1, mft_full = mft_dec == 0;
	real LB[N * N], dB[N], z[6];
	for (int i = 0; i < 6; i++) z[i] = Fu[i];
	if (mft_bie || jt_dec == 1) {
		real MB[N * N];
		for (int i = 0; i < N * N; i++) MB[i] = M[i];
		for (int i = 0; i < N; i++) MB[i * N + i] = std::fmax(MB[i * N + i], thr);
		chol<N>(MB, LB, dB);
	}
	if (mft_bie) {
		real YB[N * 6], AB[36], LAB[36], dAB[6];
		whitened(LB, dB, J, YB, AB, LAB, dAB);
		solve_lower<6>(LAB, dAB, z);
		solve_lower_t<6>(LAB, dAB, z);
	}
	real L[N * N], dL[N], Y[N * 6], A[36], LA[36], dA[6];
	chol<N>(M, L, dL);
	whitened(L, dL, J, Y, A, LA, dA);
	if (mft_full) {
		solve_lower<6>(LA, dA, z);
		solve_lower_t<6>(LA, dA, z);
	}
	real a[N], bb[N], na2 = 0, w[N];
	{
		real tk[6] = {0, 0, 0, 0, 0, 0}, best = -1;
		int ks = 0;
		for (int i = 0; i < N; i++) {
			real t[6];
			for (int c = 0; c < 6; c++) t[c] = Y[i * 6 + c];
			solve_lower<6>(LA, dA, t);
			real pd = 1.0;
			for (int c = 0; c < 6; c++) pd = std::fma(-t[c], t[c], pd);
			if (pd > best) {
				best = pd, ks = i;
				for (int c = 0; c < 6; c++) tk[c] = t[c];
			}
		}
		solve_lower_t<6>(LA, dA, tk);
		const real wn = 1.0 / std::sqrt(best);
		for (int i = 0; i < N; i++) {
			real s = (ks == i) ? 1.0 : 0.0;
			for (int c = 0; c < 6; c++) s = std::fma(-Y[i * 6 + c], tk[c], s);
			w[i] = s * wn;
		}
		real cw[6], nn = 0;
		for (int c = 0; c < 6; c++) {
			real s = 0;
			for (int i = 0; i < N; i++) s = std::fma(Y[i * 6 + c], w[i], s);
			cw[c] = s;
		}
		solve_lower<6>(LA, dA, cw);
		solve_lower_t<6>(LA, dA, cw);
		for (int i = 0; i < N; i++) {
			real s = w[i];
			for (int c = 0; c < 6; c++) s = std::fma(-Y[i * 6 + c], cw[c], s);
			w[i] = s;
			nn = std::fma(s, s, nn);
		}
		const real rn = 1.0 / std::sqrt(nn);
		for (int i = 0; i < N; i++) w[i] *= rn;
	}
	for (int i = 0; i < N; i++) a[i] = w[i];
	solve_lower_t<N>(L, dL, a);
	for (int i = 0; i < N; i++) {
		real s = 0;
		for (int k = 0; k <= i; k++) s = std::fma(L[i * N + k], w[k], s);
		bb[i] = s;
	}
	for (int i = 0; i < N; i++) na2 = std::fma(a[i], a[i], na2);
	for (int i = 0; i < 6; i++) z[i] += Ff[i];
	real yz[N], tau_mft[N];
	for (int i = 0; i < N; i++) {
		real s = 0;
		for (int c = 0; c < 6; c++) s = std::fma(Y[i * 6 + c], z[c], s);
		yz[i] = s;
	}
	for (int i = 0; i < N; i++) {
		real s = 0;
		for (int k = 0; k <= i; k++) s = std::fma(L[i * N + k], yz[k], s);
		tau_mft[i] = s;
	}
	real af = 0, aacc = 0;
	jt.project(a, af, aacc);
	if (with_comp) {
		real u[N];
		for (int i = 0; i < N; i++) u[i] = yz[i];
		solve_lower_t<N>(L, dL, u);
		for (int i = 0; i < N; i++) aacc = std::fma(-a[i], u[i], aacc);
	}
	real coef = aacc / na2;
	if (jt_dec == 0) {
		coef += af / na2;
	} else if (jt_dec == 2) {
		coef += af;
	} else {
		real y[N], beta = 0;
		for (int i = 0; i < N; i++) y[i] = bb[i];
		solve_lower<N>(LB, dB, y);
		for (int i = 0; i < N; i++) beta = std::fma(y[i], y[i], beta);
		coef += af / (beta * na2);
	}
	for (int i = 0; i < N; i++) {
		tau[i] = std::fma(bb[i], coef, tau_mft[i]);
		pr.tau_mft[i] = tau_mft[i], pr.a[i] = a[i], pr.bb[i] = bb[i];
	}
}

bool read(real* x, int n) {
	for (int i = 0; i < n; i++)
		if (std::scanf("%lf", x + i) != 1) return false;
	return true;
}
void row(const char* tag, const sai2b::chain::Probe& pr, const real* tau) {
	std::printf("%s", tag);
	for (int i = 0; i < N; i++) std::printf(" %.17g", pr.tau_mft[i]);
	for (int i = 0; i < N; i++) std::printf(" %.17g", pr.a[i]);
	for (int i = 0; i < N; i++) std::printf(" %.17g", pr.bb[i]);
	for (int i = 0; i < N; i++) std::printf(" %.17g", tau[i]);
	std::printf("\n");
}
}  // namespace

int main() {
	real J[6 * N], M[N * N], Fu[6], Ff[6], f[N], ddq[N], sw[4];
	int cases = 0;
	while (read(J, 6 * N)) {
		if (!(read(M, N * N) && read(Fu, 6) && read(Ff, 6) && read(f, N) && read(ddq, N) && read(sw, 4))) {
			std::fprintf(stderr, "case %d is cut short\n", cases);
			return 2;
		}
		const int mft_dec = (int)sw[0], jt_dec = (int)sw[1];
		const real thr = sw[2];
		const bool comp = sw[3] != 0;
		real tau[N];
		sai2b::chain::Probe pr;
		Law law{f, ddq};
		sai2b::chain::tick2<N>(J, M, Fu, Ff, mft_dec == 1, mft_dec == 0, jt_dec == 0, jt_dec == 2, thr, comp, law, tau, &pr);
		if (law.prefetched != 11) return 3;
		row("new", pr, tau);
		Law law2{f, ddq};
		old_tick(J, M, Fu, Ff, mft_dec, jt_dec, thr, comp, law2, tau, pr);
		row("old", pr, tau);
		cases++;
	}
	std::fprintf(stderr, "%d cases\n", cases);
	return cases ? 0 : 1;
}

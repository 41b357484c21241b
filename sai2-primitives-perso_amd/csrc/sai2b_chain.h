// sai2b_chain.h — the whitened factor chain of the [full MotionForceTask, full JointTask] fast tick (sai2b_fast.hpp),
// as routines on plain arrays. No HIP in here: under hipcc they are __host__ __device__, elsewhere inline, so
// tests/cpp/chain_driver.cpp runs the same code on a CPU against a 40-digit reference.
//
// For an SPD n x n matrix Mx (M itself, or M with its diagonal raised to the bounded-inertia threshold) and the 6 x n
// Jacobian J:
//     Mx = Lx Lx^T,   Yx = Lx^-1 J^T  (n x 6),   Yx = Q [R; 0]   (Householder, Q n x n orthogonal, R 6 x 6 upper)
// so J Mx^-1 J^T = Yx^T Yx = R^T R: the operational-space solves run on R, which is what a Cholesky factor of the Gram
// matrix would be, without forming the Gram matrix. And with n = 7 the last column of Q is the one direction orthogonal
// to range(Yx):  w = Q e_6,  Yx^T w = [R^T 0] Q^T Q e_6 = 0. w is a product of six reflectors applied to a unit vector,
// so it is orthogonal to range(Yx) to rounding whatever the conditioning of Yx: no search for a well-conditioned row of
// the complementary projector and no re-orthogonalisation (a Gram matrix squares the condition number; this does not).
//
// Nullspace. N = I - M^-1 J^T (J M^-1 J^T)^-1 J is the projector onto null(J) along range(M^-1 J^T). null(J) is
// one-dimensional, so N = nv c^T for any nv in null(J), with c^T nv = 1 and c^T M^-1 J^T = 0, i.e. M^-1 c in null(J):
// c = M nv / (nv^T M nv). Hence
//     N = nv (M nv)^T / (nv^T M nv)          for ANY nv in null(J),
// and nv = Lx^-T w qualifies for any SPD factor Lx (J nv = Yx^T w = 0), the bounded-inertia one included: the nullspace
// needs no chain of its own on M. The tick wants a = nv / sqrt(s), bb = M nv / sqrt(s), s = nv^T M nv (a^T M a = 1).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SAI2B_HD __host__ __device__ __forceinline__
#else
#define SAI2B_HD inline
#endif
#if defined(__clang__)
#define SAI2B_CHAIN_UNROLL _Pragma("unroll")
#else
#define SAI2B_CHAIN_UNROLL
#endif
#ifndef SAI2B_CHAIN_PHASE  // a scheduling fence between phases, where the includer has one (sai2b_fast.hpp)
#define SAI2B_CHAIN_PHASE() do { } while (0)
#endif

namespace sai2b {
namespace chain {

typedef double real;

SAI2B_HD real rsqrt_(real x) {
#if defined(__HIP_DEVICE_COMPILE__)
	return ::rsqrt(x);
#else
	return 1.0 / std::sqrt(x);
#endif
}
// 1 / x for a positive, well-scaled x (a product of two column norms): the hardware seed and two Newton steps
SAI2B_HD real rcp_(real x) {
#if defined(__HIP_DEVICE_COMPILE__)
	real r = __builtin_amdgcn_rcp(x);
	r = fma(fma(-x, r, 1.0), r, r);
	return fma(fma(-x, r, 1.0), r, r);
#else
	return 1.0 / x;
#endif
}

// Cholesky factor of M (raise = false) or of M with every diagonal element raised to at least thr (raise = true):
// lower L, row-major, upper part untouched, and the reciprocals of its diagonal. M is anything indexed [i * n + j]
// for j <= i.
template <int n, class Mat>
SAI2B_HD void chol_sel(const Mat& M, bool raise, real thr, real* L, real* dinv) {
	SAI2B_CHAIN_UNROLL for (int j = 0; j < n; j++) {
		const real mjj = M[j * n + j];
		real s = raise ? fmax(mjj, thr) : mjj;
		SAI2B_CHAIN_UNROLL for (int k = 0; k < j; k++) s = fma(-L[j * n + k], L[j * n + k], s);
		const real r = rsqrt_(s);
		dinv[j] = r;
		L[j * n + j] = s * r;
		SAI2B_CHAIN_UNROLL for (int i = j + 1; i < n; i++) {
			real t = M[i * n + j];
			SAI2B_CHAIN_UNROLL for (int k = 0; k < j; k++) t = fma(-L[i * n + k], L[j * n + k], t);
			L[i * n + j] = t * r;
		}
	}
}
// x <- L^-1 x
template <int n>
SAI2B_HD void fwd(const real* L, const real* dinv, real* x) {
	SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) {
		real t = x[i];
		SAI2B_CHAIN_UNROLL for (int k = 0; k < i; k++) t = fma(-L[i * n + k], x[k], t);
		x[i] = t * dinv[i];
	}
}
// x <- L^-T x
template <int n>
SAI2B_HD void bwd(const real* L, const real* dinv, real* x) {
	SAI2B_CHAIN_UNROLL for (int i = n - 1; i >= 0; i--) {
		real t = x[i];
		SAI2B_CHAIN_UNROLL for (int k = i + 1; k < n; k++) t = fma(-L[k * n + i], x[k], t);
		x[i] = t * dinv[i];
	}
}

// Y = L^-1 J^T: J is 6 x n row-major, Y is n x 6 row-major
template <int n>
SAI2B_HD void whiten(const real* L, const real* dinv, const real* J, real* Y) {
	SAI2B_CHAIN_UNROLL for (int c = 0; c < 6; c++) {
		real col[n];
		SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) col[i] = J[c * n + i];
		fwd<n>(L, dinv, col);
		SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) Y[i * 6 + c] = col[i];
	}
}

// Householder QR of the n x 6 matrix Y, in place, n > 6. Reflector k is H_k = I - beta[k] v_k v_k^T on rows k .. n-1,
// with v_k = x - alpha e_0 for the column x it clears, alpha = -copysign(|x|, x_0) (no cancellation in v_k[0]) and
// beta = 2 / v^T v = 1 / (|x| (|x| + |x_0|)). On return Y[i * 6 + k], i >= k, holds v_k; Y[k * 6 + j], j > k, holds
// R[k][j]; rdiag[k] = R[k][k] = alpha and rinv[k] = 1 / alpha. Straight-line: nothing here depends on the data but
// copysign.
template <int n>
SAI2B_HD void qr6(real* Y, real* rdiag, real* rinv, real* beta) {
	SAI2B_CHAIN_UNROLL for (int k = 0; k < 6; k++) {
		real ss = 0;
		SAI2B_CHAIN_UNROLL for (int i = k; i < n; i++) ss = fma(Y[i * 6 + k], Y[i * 6 + k], ss);
		const real rs = rsqrt_(ss), nrm = ss * rs, x0 = Y[k * 6 + k];
		const real v0 = x0 + copysign(nrm, x0);
		rdiag[k] = -copysign(nrm, x0);
		rinv[k] = -copysign(rs, x0);
		const real bk = rcp_(nrm * fabs(v0));
		beta[k] = bk;
		Y[k * 6 + k] = v0;
		SAI2B_CHAIN_UNROLL for (int j = k + 1; j < 6; j++) {
			real d = 0;
			SAI2B_CHAIN_UNROLL for (int i = k; i < n; i++) d = fma(Y[i * 6 + k], Y[i * 6 + j], d);
			d *= bk;
			SAI2B_CHAIN_UNROLL for (int i = k; i < n; i++) Y[i * 6 + j] = fma(-d, Y[i * 6 + k], Y[i * 6 + j]);
		}
	}
}

// z <- R^-T z, from qr6's output (R^T is lower: forward substitution)
SAI2B_HD void solve_rt(const real* Y, const real* rinv, real* z) {
	SAI2B_CHAIN_UNROLL for (int i = 0; i < 6; i++) {
		real t = z[i];
		SAI2B_CHAIN_UNROLL for (int k = 0; k < i; k++) t = fma(-Y[k * 6 + i], z[k], t);
		z[i] = t * rinv[i];
	}
}
// z <- R z
SAI2B_HD void mul_r(const real* Y, const real* rdiag, real* z) {
	SAI2B_CHAIN_UNROLL for (int i = 0; i < 6; i++) {
		real t = rdiag[i] * z[i];
		SAI2B_CHAIN_UNROLL for (int k = i + 1; k < 6; k++) t = fma(Y[i * 6 + k], z[k], t);
		z[i] = t;
	}
}
// x <- Q [x_0 .. x_5; 0] = H_0 ... H_5 [x; 0]: on entry x[0 .. 5], on return all n rows (n = 7). Row n - 1 is still zero
// when H_5 is applied, so it is left out of that dot product.
template <int n>
SAI2B_HD void apply_q(const real* Y, const real* beta, real* x) {
	static_assert(n == 7, "one row below R");
	SAI2B_CHAIN_UNROLL for (int k = 5; k >= 0; k--) {
		real d = 0;
		SAI2B_CHAIN_UNROLL for (int i = k; i < (k == 5 ? n - 1 : n); i++) d = fma(Y[i * 6 + k], x[i], d);
		d *= beta[k];
		SAI2B_CHAIN_UNROLL for (int i = k; i < n; i++) {
			if (k == 5 && i == n - 1)
				x[i] = -d * Y[i * 6 + k];
			else
				x[i] = fma(-d, Y[i * 6 + k], x[i]);
		}
	}
}

// w = Q e_{n-1} = H_0 ... H_5 e_{n-1}: the reflectors in reverse order on the last unit vector. Before H_k is applied
// rows 0 .. k are still zero, so they are left out of its dot product.
template <int n>
SAI2B_HD void null_w(const real* Y, const real* beta, real* w) {
	SAI2B_CHAIN_UNROLL for (int i = 0; i < n - 1; i++) w[i] = 0;
	w[n - 1] = 1.0;
	SAI2B_CHAIN_UNROLL for (int k = 5; k >= 0; k--) {
		real d = 0;
		SAI2B_CHAIN_UNROLL for (int i = (k == 5 ? n - 1 : k + 1); i < n; i++) d = fma(Y[i * 6 + k], w[i], d);
		d *= beta[k];
		w[k] = -d * Y[k * 6 + k];
		SAI2B_CHAIN_UNROLL for (int i = k + 1; i < n; i++) {
			if (k == 5 && i < n - 1)
				w[i] = -d * Y[i * 6 + k];
			else
				w[i] = fma(-d, Y[i * 6 + k], w[i]);
		}
	}
}

// The nullspace pair from w: nv = L^-T w, m = M nv (M symmetric, its lower triangle is read), s = nv . m;
// a = nv / sqrt(s), bb = m / sqrt(s), na2 = |a|^2. Then N = a bb^T and a^T M a = 1.
template <int n, class Mat>
SAI2B_HD void null_pair(const real* L, const real* dinv, const real* w, const Mat& M, real* a, real* bb, real& na2) {
	real nv[n], m[n];
	SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) nv[i] = w[i];
	bwd<n>(L, dinv, nv);
	SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) m[i] = 0;
	SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) SAI2B_CHAIN_UNROLL for (int j = 0; j <= i; j++) {
		const real mij = M[i * n + j];
		m[i] = fma(mij, nv[j], m[i]);
		if (j < i) m[j] = fma(mij, nv[i], m[j]);
	}
	real s = 0;
	SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) s = fma(nv[i], m[i], s);
	const real rs = rsqrt_(s);
	na2 = 0;
	SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) {
		a[i] = nv[i] * rs;
		bb[i] = m[i] * rs;
		na2 = fma(a[i], a[i], na2);
	}
}

// What a test may want to see of tick2 besides the torques
struct Probe {
	real tau_mft[8], a[8], bb[8];
};

// The two-level tick behind the model phase and the MotionForceTask law (closed forms: top of sai2b_fast.hpp).
// J (6 x n) and M at q, Fu / Ff the task forces of the MotionForceTask law, thr the bounded-inertia threshold;
// mft_bie / mft_full and jt_full / jt_imp name the tasks' decoupling (neither: impedance for the MotionForceTask,
// bounded inertia for the JointTask). jt gives the JointTask law: prefetch() is called first and prefetch_q() behind
// the QR (what they load is the caller's business), project(a, af, aacc) adds a . f and a . ddq once a exists.
// One chain, on Mx = Mb when the MotionForceTask is bounded-inertia and on M otherwise. The other factor is needed only
// for a^T M^-1 tau_mft (chain on Mb, with_comp) or for beta = bb^T Mb^-1 bb (chain on M, bounded-inertia JointTask):
// at most one further Cholesky, behind a batch-uniform branch.
template <int n, class Mat, class JT>
SAI2B_HD void tick2(const real* J, const Mat& M, const real* Fu, const real* Ff, bool mft_bie, bool mft_full, bool jt_full,
					bool jt_imp, real thr, bool with_comp, JT& jt, real* tau, Probe* probe = nullptr) {
	jt.prefetch();
	SAI2B_CHAIN_PHASE();
	real Lx[n * n], dx[n], Y[n * 6], rdiag[6], rinv[6], beta[6];
	chol_sel<n>(M, mft_bie, thr, Lx, dx);
	whiten<n>(Lx, dx, J, Y);
	SAI2B_CHAIN_PHASE();
	qr6<n>(Y, rdiag, rinv, beta);
	jt.prefetch_q();
	// MotionForceTask torques J^T (Lambda_mod F_unit + F_force)   (SingularityHandler.cpp:307-309), through the chain: J^T =
	// Lx Yx = Lx Q [R; 0] and Lambda_mod = (J Mx^-1 J^T)^-1 = R^-1 R^-T, so J^T Lambda_mod F_unit = Lx Q [R^-T F_unit; 0]
	// (half of the solve cancels) and J^T F_force = Lx Q [R F_force; 0]. Lambda_mod = I (impedance): R F_unit instead.
	real yz[n], tau_mft[n];
	{
		real rf[6];
		SAI2B_CHAIN_UNROLL for (int i = 0; i < 6; i++) yz[i] = Fu[i], rf[i] = Ff[i];
		if (mft_bie || mft_full)
			solve_rt(Y, rinv, yz);
		else
			mul_r(Y, rdiag, yz);
		mul_r(Y, rdiag, rf);
		SAI2B_CHAIN_UNROLL for (int i = 0; i < 6; i++) yz[i] += rf[i];
		apply_q<n>(Y, beta, yz);  // Yx (Lambda_mod F_unit + F_force) = Lx^-1 tau_mft
		SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) {
			real s = 0;
			SAI2B_CHAIN_UNROLL for (int k = 0; k <= i; k++) s = fma(Lx[i * n + k], yz[k], s);
			tau_mft[i] = s;
		}
	}
	real a[n], bb[n], na2;
	{
		real w[n];
		null_w<n>(Y, beta, w);
		null_pair<n>(Lx, dx, w, M, a, bb, na2);
	}
	SAI2B_CHAIN_PHASE();
	// JointTask: its law enters only as a . f and a . ddq
	real af = 0, aacc = 0;
	jt.project(a, af, aacc);
	const bool jt_bie = !jt_full && !jt_imp;
	real LO[n * n], dO[n];
	if (mft_bie ? with_comp : jt_bie) chol_sel<n>(M, !mft_bie, thr, LO, dO);
	if (with_comp) {  // JointTask.cpp:285-292: - Jp^T R M_partial R^T S M^-1 tau_prec
		real u[n];
		SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) u[i] = tau_mft[i];
		if (mft_bie) {
			fwd<n>(LO, dO, u);
			bwd<n>(LO, dO, u);
		} else {  // M^-1 tau_mft = Lx^-T (Lx^-1 tau_mft)
			SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) u[i] = yz[i];
			bwd<n>(Lx, dx, u);
		}
		SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) aacc = fma(-a[i], u[i], aacc);
	}
	real coef = aacc / na2;	 // a^T (a a^T / |a|^4) v = (a.v) / |a|^2
	if (jt_full) {
		coef += af / na2;
	} else if (jt_imp) {
		coef += af;	 // a^T (a a^T / |a|^2) f
	} else {
		real y[n];
		SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) y[i] = bb[i];
		if (mft_bie)
			fwd<n>(Lx, dx, y);
		else
			fwd<n>(LO, dO, y);
		real bt = 0;  // beta = bb^T Mb^-1 bb
		SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) bt = fma(y[i], y[i], bt);
		coef += af / (bt * na2);
	}
	SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) tau[i] = fma(bb[i], coef, tau_mft[i]);  // Jp^T x = b (a^T x)
	if (probe) {
		SAI2B_CHAIN_UNROLL for (int i = 0; i < n; i++) probe->tau_mft[i] = tau_mft[i], probe->a[i] = a[i], probe->bb[i] = bb[i];
	}
}

}  // namespace chain
}  // namespace sai2b

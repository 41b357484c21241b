// sai2b_rng.h — the library's counter-based random generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC'11), written from its definition, and unit normals from its words by Box-Muller.
// A draw is a pure function of (counter, key): nothing is stored between draws, so a robot's noise does not depend on the
// batch it runs in, on the order of launches or on what other robots do, and a saved counter reproduces it.
// No HIP in here when a host compiler reads it: tests/cpp/hardware_driver.cpp runs the same code on a CPU.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SAI2B_RNG_HD __host__ __device__
#else
#define SAI2B_RNG_HD
#endif

namespace sai2b {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;  // the two round multipliers
constexpr unsigned PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;  // the key schedule's increments (golden ratio, sqrt 3 - 1)

// x[4]: the counter on entry, the four output words on return. Ten rounds; the key is bumped between rounds. A round is two
// 32 x 32 -> 64 products (mul_hi / mul_lo pairs on the VALU) and three XORs.
SAI2B_RNG_HD inline void philox4x32_10(unsigned x[4], unsigned k0, unsigned k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int r = 0; r < 10; r++) {
		const unsigned long long p0 = (unsigned long long)PHILOX_M0 * x[0], p1 = (unsigned long long)PHILOX_M1 * x[2];
		const unsigned y0 = (unsigned)(p1 >> 32) ^ x[1] ^ k0, y2 = (unsigned)(p0 >> 32) ^ x[3] ^ k1;
		x[1] = (unsigned)p1, x[3] = (unsigned)p0;
		x[0] = y0, x[2] = y2;
		k0 += PHILOX_W0, k1 += PHILOX_W1;
	}
}

// two unit normals from two words: u = (x + 0.5) 2^-32 lies in (0, 1) for every word, so the logarithm is finite and
// |z| <= sqrt(-2 ln 2^-33) = 6.77
SAI2B_RNG_HD inline void box_muller(unsigned x0, unsigned x1, double& z0, double& z1) {
	const double u0 = ((double)x0 + 0.5) * 2.3283064365386963e-10, u1 = ((double)x1 + 0.5) * 2.3283064365386963e-10;
	const double r = sqrt(-2.0 * log(u0)), a = 6.283185307179586 * u1;
	z0 = r * cos(a), z1 = r * sin(a);
}

// the four normals of call `call` of a stream: counter (n, e, 256 stream + call, robot), key (seed low, seed high)
SAI2B_RNG_HD inline void normals4(unsigned n, unsigned e, unsigned stream, unsigned call, unsigned robot, unsigned k0, unsigned k1, double z[4]) {
	unsigned x[4] = {n, e, 256u * stream + call, robot};
	philox4x32_10(x, k0, k1);
	box_muller(x[0], x[1], z[0], z[1]);
	box_muller(x[2], x[3], z[2], z[3]);
}

}  // namespace sai2b

// hardware_driver.cpp — the device random generator of csrc/sai2b_rng.h on a CPU. The header alone is included: built with
// plain g++, no HIP, no GPU.
//
//   hardware_driver words < lines of "c0 c1 c2 c3 k0 k1" (hex)
//       per line "x0 x1 x2 x3 z0 z1 z2 z3": the four words of Philox4x32-10 (hex) and the four normals Box-Muller makes of them
//   hardware_driver box < lines of "x0 x1" (hex)
//       per line "z0 z1": the two normals Box-Muller makes of the two words
//   hardware_driver normals n e stream call robot seed
//       "z0 z1 z2 z3" of that call as the kernels draw it
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sai2b_rng.h"

int main(int argc, char** argv) {
	if (argc == 2 && !std::strcmp(argv[1], "words")) {
		unsigned c[4], k[2];
		while (std::scanf("%x %x %x %x %x %x", &c[0], &c[1], &c[2], &c[3], &k[0], &k[1]) == 6) {
			sai2b::philox4x32_10(c, k[0], k[1]);
			double z[4];
			sai2b::box_muller(c[0], c[1], z[0], z[1]);
			sai2b::box_muller(c[2], c[3], z[2], z[3]);
			std::printf("%08x %08x %08x %08x %.17g %.17g %.17g %.17g\n", c[0], c[1], c[2], c[3], z[0], z[1], z[2], z[3]);
		}
		return 0;
	}
	if (argc == 2 && !std::strcmp(argv[1], "box")) {
		unsigned x[2];
		while (std::scanf("%x %x", &x[0], &x[1]) == 2) {
			double z[2];
			sai2b::box_muller(x[0], x[1], z[0], z[1]);
			std::printf("%.17g %.17g\n", z[0], z[1]);
		}
		return 0;
	}
	if (argc == 8 && !std::strcmp(argv[1], "normals")) {
		unsigned long long v[6];
		for (int i = 0; i < 6; i++) v[i] = std::strtoull(argv[2 + i], nullptr, 0);
		double z[4];
		sai2b::normals4((unsigned)v[0], (unsigned)v[1], (unsigned)v[2], (unsigned)v[3], (unsigned)v[4], (unsigned)(v[5] & 0xffffffffull),
						(unsigned)(v[5] >> 32), z);
		std::printf("%.17g %.17g %.17g %.17g\n", z[0], z[1], z[2], z[3]);
		return 0;
	}
	std::fprintf(stderr, "usage: hardware_driver words < counters | box < words | normals n e stream call robot seed\n");
	return 2;
}

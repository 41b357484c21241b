// joint_sensor_driver.cpp — the joint sensors' law (csrc/sai2b_joint_sensor_law.h) on a CPU: the same code joint_sense_kernel
// runs per lane, here per record with stride 1. The header alone is included: built with plain g++ (-ffp-contract=off), no HIP,
// no GPU.
//
//   joint_sensor_driver readings <ints.i32> <values.f64> <out.f64>
//       records of 8 ints (dof, m, e, velocity_mode, D, robot, key0, key1) and IN doubles, every array in a slot sized for 8
//       joints and D = 8 and packed from its start for fewer: rows 41, q 8, dq 8, dt 1, pprev 8, v 8, history 144, q_meas 8,
//       dq_meas 8, save_pose 1;
//       per record OUT doubles: pprev 8, v 8, history 144, q_meas 8, dq_meas 8, q_pose 8 (zeros unless save_pose)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sai2b_joint_sensor_law.h"

using namespace sai2b;

constexpr int INTS = 8, IN = 41 + 8 + 8 + 1 + 8 + 8 + 144 + 8 + 8 + 1, OUT = 8 + 8 + 144 + 8 + 8 + 8;

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
	const double *rows = in, *q = in + 41, *dq = in + 49, dt = in[57];
	double *prev = o, *filt = o + 8, *hist = o + 16, *qm = o + 160, *dqm = o + 168, *pose = o + 176;
	std::memcpy(prev, in + 58, 8 * sizeof(double));
	std::memcpy(filt, in + 66, 8 * sizeof(double));
	std::memcpy(hist, in + 74, 144 * sizeof(double));
	std::memcpy(qm, in + 218, 8 * sizeof(double));
	std::memcpy(dqm, in + 226, 8 * sizeof(double));
	const bool draw = joint_sensor_noisy<DOF>(rows, 1);
	joint_sensor_reading<DOF>(rows, 1, q, dq, dt, c[1], c[2], c[3], c[4], draw, (unsigned)c[6], (unsigned)c[7], (unsigned)c[5], prev, filt, hist, qm,
							  dqm, in[234] != 0.0 ? pose : nullptr);
}

int main(int argc, char** argv) {
	if (argc != 5 || std::strcmp(argv[1], "readings")) {
		std::fprintf(stderr, "usage: joint_sensor_driver readings <ints> <values> <out>\n");
		return 2;
	}
	std::vector<int> c;
	std::vector<double> v;
	if (!read_all(argv[2], c) || !read_all(argv[3], v) || c.size() % INTS || v.size() % IN || c.size() / INTS != v.size() / IN) return 2;
	const size_t R = c.size() / INTS;
	std::vector<double> out(OUT * R, 0.0);
	for (size_t r = 0; r < R; r++) {
		const int* k = &c[INTS * r];
		if (k[4] < 0 || k[4] > 8 || k[1] < 0) return 2;
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

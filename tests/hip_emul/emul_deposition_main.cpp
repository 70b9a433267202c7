// TEST INFRASTRUCTURE ONLY: the product's binner (rays_amd/csrc/rays_deposition.hpp: deposit_ray, Ptotal_x) as a
// stand-alone host program for sanitizer runs (tests/test_cpu_deposition_binner.py builds it with
// -fsanitize=address,undefined).  Every case is binned into a heap row of EXACTLY n_bins doubles, from heap copies of
// exactly nx points, so an access one element past a ray's row -- which the lane-interleaved LDS rows of the device
// kernel and the packed work array of emul_trace.cpp hide -- is reported.
//
//   emul_deposition_main <case file> <result file>
//
// The files are those of oracle/ref_binner_driver.f90 (tests/deposition_cases.py: write_case_file / read_result_file):
//   case file:    int32 ncase, then per case: float64 xmin, xmax; int32 n_bins, nx; float64 xQ[nx], Q[nx]
//   result file:  per case: int32 0; float64 row[n_bins]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <memory>
RAYS_EMUL_DEFINE_GLOBALS
#include "../../rays_amd/csrc/rays_deposition.hpp"

static bool get(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) { std::fprintf(stderr, "cannot open the case / result file\n"); return 2; }
  int32_t ncase = 0;
  if (!get(in, &ncase, 4)) return 3;
  const rays::DevParams P{};   // Ptotal_x reads nothing of it
  for (int32_t c = 0; c < ncase; c++) {
    double lim[2];
    int32_t dims[2];
    if (!get(in, lim, 16) || !get(in, dims, 8) || dims[0] < 1 || dims[1] < 0) return 3;
    const int n_bins = dims[0], nx = dims[1];
    constexpr int nv = 8;
    std::unique_ptr<double[]> xq(new double[nx]), q(new double[nx]), rv(new double[(size_t)nx * nv]()),
        row(new double[n_bins]);
    if (!get(in, xq.get(), 8 * (size_t)nx) || !get(in, q.get(), 8 * (size_t)nx)) return 3;
    for (int i = 0; i < nx; i++) { rv[(size_t)i * nv] = xq[i]; rv[(size_t)i * nv + 7] = q[i]; }
    const int32_t np = nx;
    const double power = 1.0;   // q = ray_vec(8) * 1: the case's Q itself
    rays::DepArgs A{};
    A.which = 2; A.n_bins = n_bins; A.nray = 1; A.nv = nv; A.npt = nx;
    A.grid_min = lim[0]; A.grid_max = lim[1];
    A.ray_vec = rv.get(); A.npoints = &np; A.power = &power; A.work = nullptr;
    rays::deposit_ray(P, A, 0, row.get(), 1);
    const int32_t zero = 0;
    std::fwrite(&zero, 4, 1, out);
    std::fwrite(row.get(), 8, (size_t)n_bins, out);
  }
  if (std::fclose(out) != 0) return 4;
  std::fclose(in);
  return 0;
}

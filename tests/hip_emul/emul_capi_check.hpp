// TEST INFRASTRUCTURE ONLY: what the stand-alone programs of this directory (emul_*_main.cpp) share -- the counted
// CHECK, the case-file reader, refusals by message, and the oracle's case with its two comparisons.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rays_hip.h"

inline int failures = 0;
#define CHECK(cond) \
  do { if (!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

template <class T>
inline bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
inline std::string last_error() {
  char buf[512];
  rays_hip_last_error(buf, (int)sizeof buf);
  return buf;
}
inline bool refused(int rc, const char* text) {
  const bool ok = rc != 0 && last_error().find(text) != std::string::npos;
  if (!ok) std::fprintf(stderr, "expected a refusal with \"%s\", got rc %d: %s\n", text, rc, last_error().c_str());
  return ok;
}

// the oracle's case: summaries and packed trajectories (offs[i]: first packed point of ray i)
struct Case {
  size_t nv = 0, npt = 0;
  std::vector<int32_t> np, sc;
  std::vector<double> end, eres, mres, pv, pr;
  std::vector<size_t> offs;
};
// ray_vec[n][npt][nv] / residual[n][npt] of the first n rays: points 1..npoints are the oracle's bit for bit, every
// slot behind them holds `rest` (the poison the entry must not overwrite, or the zeros of a gathered result)
inline bool same_trajectories(const Case& c, size_t n, const double* rv, const double* res, double rest) {
  for (size_t i = 0; i < n; i++) {
    const size_t k = (size_t)c.np[i];
    if (std::memcmp(rv + c.npt * c.nv * i, c.pv.data() + c.offs[i] * c.nv, sizeof(double) * c.nv * k) != 0 ||
        std::memcmp(res + c.npt * i, c.pr.data() + c.offs[i], sizeof(double) * k) != 0)
      return false;
    for (size_t j = k * c.nv; j < c.npt * c.nv; j++)
      if (std::memcmp(&rv[c.npt * c.nv * i + j], &rest, sizeof rest) != 0) return false;
    for (size_t j = k; j < c.npt; j++)
      if (std::memcmp(&res[c.npt * i + j], &rest, sizeof rest) != 0) return false;
  }
  return true;
}
inline bool same_summaries(const Case& c, size_t n, const int32_t* np, const int32_t* sc, const double* end,
                           const double* er, const double* mr) {
  return std::memcmp(np, c.np.data(), sizeof(int32_t) * n) == 0 && std::memcmp(sc, c.sc.data(), sizeof(int32_t) * n) == 0 &&
         std::memcmp(end, c.end.data(), sizeof(double) * c.nv * n) == 0 &&
         std::memcmp(er, c.eres.data(), sizeof(double) * n) == 0 && std::memcmp(mr, c.mres.data(), sizeof(double) * n) == 0;
}

// Host build of the chain's random numbers (quantpy_amd/csrc/qt_sampler.h: mhmc_draw) for
// tests/test_mhmc_coverage_host.py and tests/test_gpu_mhmc_coverage.py: the same function the kernels call, compiled by
// g++ with the host libm.  Test infrastructure, not product.
#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC diagnostic ignored "-Wunknown-pragmas"
#endif
#include "../../quantpy_amd/csrc/qt_sampler.h"

extern "C" {
// deltas[C][T][D], uniforms[C][T] of chains first_chain .., steps first_step ..  (the table of qt_mhmc_draws)
void qt_host_mhmc_draws(uint64_t seed, uint64_t first_chain, int C, uint32_t first_step, int T, int D, double* deltas,
                        double* uniforms) {
  for (int c = 0; c < C; ++c)
    for (int t = 0; t < T; ++t) {
      const size_t ct = (size_t)c * T + t;
      for (int l = 0; l < D; ++l)
        deltas[ct * D + l] = qt_sampler::mhmc_draw(seed, first_chain + (uint64_t)c, first_step + (uint32_t)t, D, l);
      uniforms[ct] = qt_sampler::mhmc_draw(seed, first_chain + (uint64_t)c, first_step + (uint32_t)t, D, D);
    }
}
}

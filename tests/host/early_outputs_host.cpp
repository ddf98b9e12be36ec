// Host build of the start-point rules of quantpy_amd/csrc/qt_linesearch.h for tests/test_early_outputs_host.py only.
#include "../../quantpy_amd/csrc/qt_linesearch.h"
extern "C" {
int qt_host_start_status(int shots_ok, int ok, int iterate, int max_iter, double gnorm, double fk, int xnan) {
  return qt::mle_start_status(shots_ok != 0, ok != 0, iterate != 0, max_iter, gnorm, fk, xnan != 0);
}
int qt_host_early_scalars_final(int shots_ok, int ok, int iterate, int max_iter, double gnorm, double fk, int xnan,
                                int fun_wanted) {
  return qt::mle_early_scalars_final(shots_ok != 0, ok != 0, iterate != 0, max_iter, gnorm, fk, xnan != 0,
                                     fun_wanted != 0)
             ? 1
             : 0;
}
}

// Host build of quantpy_amd/csrc/qt_linesearch.h for tests/test_linesearch_host.py only.
#include "../../quantpy_amd/csrc/qt_linesearch.h"
extern "C" {
typedef void (*phi_cb)(double alpha, double* f, double* g);
// returns 1 accepted / 0 failed; *stp, *fval, *nevals out; mode_out = searcher mode at exit
int qt_host_line_search(phi_cb cb, double phi0, double old_phi0, double derphi0, double* stp_out,
                        double* f_out, int* nevals, int* mode_out) {
  qt::LineSearch ls;
  double stp;
  int r = ls.start(phi0, old_phi0, derphi0, &stp);
  int n = 0;
  double f = phi0, g = derphi0;
  while (r == qt::LS_EVAL && n < 400) {
    cb(stp, &f, &g);
    ++n;
    double next = stp;
    r = ls.advance(stp, f, g, &next);
    if (r == qt::LS_EVAL) stp = next;
  }
  *stp_out = stp;
  *f_out = f;
  *nevals = n;
  *mode_out = ls.mode;
  return r == qt::LS_ACCEPT ? 1 : 0;
}

// the scalar rules around the line search, as the kernels call them
int qt_host_eval_cap(int max_iter) { return qt::bfgs_eval_cap(max_iter); }
double qt_host_rho(double ys) { return qt::bfgs_rho(ys); }
// returns 1 stop / 0 go; *status in: what the loop holds (0), out: what the exit made of it
int qt_host_step_exit(double gnorm, double gtol, double stp, double pnorm2, double fk, int kiter, int max_iter,
                      int* status) {
  return qt::bfgs_step_exit(gnorm, gtol, stp, pnorm2, fk, kiter, max_iter, status) ? 1 : 0;
}
int qt_host_final_status(int status, int kiter, int max_iter, double gn, double fk, double xn) {
  return qt::bfgs_final_status(status, kiter, max_iter, gn, fk, xn);
}
int qt_host_start_status(int shots_ok, int ok, int iterate, int max_iter, double gnorm, double fk, int xnan) {
  return qt::mle_start_status(shots_ok != 0, ok != 0, iterate != 0, max_iter, gnorm, fk, xnan != 0);
}
}

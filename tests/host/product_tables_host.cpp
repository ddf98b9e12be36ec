// Stand-alone check of quantpy_amd/csrc/qt_product_tables.h (tests/test_product_tables_host.py compiles and runs it, once
// plain and once under -fsanitize=address,undefined).  Prints a line per failed check; exit status 0 when there is none.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../quantpy_amd/csrc/qt_product_tables.h"

namespace {

int g_failed = 0, g_checks = 0;
#define CHECK(cond, ...)            \
  do {                              \
    ++g_checks;                     \
    if (!(cond)) {                  \
      if (++g_failed <= 40) {       \
        printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
        printf(__VA_ARGS__);        \
        printf("\n");               \
      }                             \
    }                               \
  } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
double uniform01() {  // xorshift64*: (0, 1)
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return ((g_rng * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-17;
}

long long ipow(long long b, int e) {
  long long r = 1;
  for (int i = 0; i < e; ++i) r *= b;
  return r;
}

// Small::fwd_ints / bwd_ints (qt_small.h), restated
long long fwd_ints(int n, long long R1) {
  long long t = 0;
  for (int q = 1; q <= n; ++q) t += ipow(R1, q) * ipow(4, n - q);
  return t;
}
long long bwd_ints(int n, long long R1) {
  long long t = 0;
  for (int q = 1; q <= n; ++q) t += ipow(R1, q - 1) * ipow(4, n - q + 1);
  return t;
}

// The definition: A[s K + k][j] = prod_q T[s_q K1 + o_q][j_q], qubit 1 the most significant digit of s, k and j.
// out = A v (forward) and out = A^T y (backward), by plain nested loops over the digits.
void kron_apply(int n, int S1, int K1, const double* t1, const std::vector<double>& v, const std::vector<double>& y,
                std::vector<double>& Av, std::vector<double>& ATy) {
  const long long S = ipow(S1, n), K = ipow(K1, n), D = ipow(4, n);
  Av.assign((size_t)(S * K), 0.0);
  ATy.assign((size_t)D, 0.0);
  std::vector<int> sd(n), od(n);
  std::vector<double> row_a((size_t)D), next((size_t)D);
  for (long long s = 0; s < S; ++s)
    for (long long k = 0; k < K; ++k) {
      long long sr = s, kr = k;
      for (int q = n - 1; q >= 0; --q) {
        sd[q] = (int)(sr % S1);
        od[q] = (int)(kr % K1);
        sr /= S1;
        kr /= K1;
      }
      // the row as np.kron builds it, left to right: row <- row (x) T[s_q K1 + o_q]
      long long len = 1;
      row_a[0] = 1.0;
      for (int q = 0; q < n; ++q) {
        const double* tr = t1 + (sd[q] * K1 + od[q]) * 4;
        for (long long j = 0; j < len; ++j)
          for (int c = 0; c < 4; ++c) next[(size_t)(4 * j + c)] = row_a[(size_t)j] * tr[c];
        len *= 4;
        row_a.swap(next);
      }
      const long long row = s * K + k;
      double acc = 0.0;
      for (long long j = 0; j < D; ++j) {
        acc += row_a[(size_t)j] * v[(size_t)j];
        ATy[(size_t)j] += row_a[(size_t)j] * y[(size_t)row];
      }
      Av[(size_t)row] = acc;
    }
}

// One stage as Small::stage_value does it: (base, sel) = entry; forward: row `sel` of the table, 4 terms; backward:
// column `sel`, R1 terms; input stride 4^(n-q).
double stage_value(bool fwd, const double* tb, int R1, int ent, long long stride, const std::vector<double>& in, long long* top) {
  const int base = ent & 0xffff, sel = ent >> 16;
  const int terms = fwd ? 4 : R1;
  double acc = 0.0;
  for (int t = 0; t < terms; ++t) {
    const long long at = base + t * stride;
    if (at > *top) *top = at;
    if (at >= (long long)in.size()) return NAN;  // (reported by the caller through `top`)
    acc += (fwd ? tb[sel * 4 + t] : tb[t * 4 + sel]) * in[(size_t)at];
  }
  return acc;
}

double max_abs(const std::vector<double>& v) {
  double m = 0.0;
  for (double x : v) m = std::fabs(x) > m ? std::fabs(x) : m;
  return m;
}

void check_shape(int n, int S1, int K1, bool uniform_shots) {
  const long long R1 = (long long)S1 * K1, S = ipow(S1, n), K = ipow(K1, n), M = ipow(R1, n), D = ipow(4, n);
  std::vector<double> t1((size_t)R1 * 4), ns((size_t)S);
  for (double& x : t1) x = 2.0 * uniform01() - 1.0;
  for (double& x : ns) x = uniform_shots ? 1000.0 : std::floor(100.0 + 900.0 * uniform01());
  qt::ProductTables tb;
  const qt::TablesStatus st = qt::build_product_tables(n, S1, K1, ns.data(), t1.data(), &tb);
  CHECK(st == qt::TABLES_OK, "n=%d (%d,%d): status %d", n, S1, K1, (int)st);
  if (st != qt::TABLES_OK) return;
  CHECK(tb.shape.S == S && tb.shape.K == K && tb.shape.M == M && tb.shape.R1 == R1, "n=%d (%d,%d): shape", n, S1, K1);
  // sizes: what the kernels stage (fwd_ints, bwd_ints, M of table_ints)
  CHECK((long long)tb.fwd.size() == fwd_ints(n, R1), "n=%d R1=%lld: fwd has %zu entries", n, R1, tb.fwd.size());
  CHECK((long long)tb.bwd.size() == bwd_ints(n, R1), "n=%d R1=%lld: bwd has %zu entries", n, R1, tb.bwd.size());
  CHECK((long long)tb.rmap.size() == M && (long long)tb.rinv.size() == M && (long long)tb.wrow.size() == M, "n=%d R1=%lld: map sizes", n, R1);
  if ((long long)tb.rmap.size() != M || (long long)tb.rinv.size() != M || (long long)tb.wrow.size() != M) return;
  // rmap: a permutation of 0 .. M-1, rinv its inverse
  std::vector<char> seen((size_t)M, 0);
  bool perm = true;
  for (long long mr = 0; mr < M && perm; ++mr) {
    const int m = tb.rmap[(size_t)mr];
    perm = m >= 0 && m < M && !seen[(size_t)m];
    if (perm) {
      seen[(size_t)m] = 1;
      perm = tb.rinv[(size_t)m] == mr;
    }
  }
  CHECK(perm, "n=%d R1=%lld: rmap / rinv are not a permutation and its inverse", n, R1);
  if (!perm) return;
  // shots
  double tot = 0.0, top = 0.0;
  bool uni = true;
  for (double x : ns) {
    tot += x;
    top = x > top ? x : top;
    uni = uni && x == ns[0];
  }
  CHECK(tb.tot == tot && tb.ns_max == top && tb.uniform == uni && tb.wuni == ns[0] / tot, "n=%d R1=%lld: shot figures", n, R1);
  long long bad_w = 0;
  for (long long mr = 0; mr < M; ++mr) bad_w += tb.wrow[(size_t)mr] != ns[(size_t)(tb.rmap[(size_t)mr] / K)] / tot;
  CHECK(bad_w == 0, "n=%d R1=%lld: %lld rows with wrow != ns[s] / tot", n, R1, bad_w);
  // packing: base below 2^16, selector below 256 (and inside its table)
  long long bad_pack = 0;
  for (int e : tb.fwd) bad_pack += e < 0 || (e >> 16) >= R1 || (e >> 16) >= 256;
  for (int e : tb.bwd) bad_pack += e < 0 || (e >> 16) >= 4;
  CHECK(bad_pack == 0, "n=%d R1=%lld: %lld entries with a bad selector", n, R1, bad_pack);
  if (bad_pack) return;
  // values: the n forward stages, read through rmap, against A v; the n backward stages against A^T y
  std::vector<double> v((size_t)D), y((size_t)M), Av, ATy;
  for (double& x : v) x = 2.0 * uniform01() - 1.0;
  for (double& x : y) x = 2.0 * uniform01() - 1.0;
  kron_apply(n, S1, K1, t1.data(), v, y, Av, ATy);
  std::vector<double> in = v, out;
  size_t at = 0;
  long long top_index = 0, size_bad = 0;
  for (int q = 1; q <= n; ++q) {
    const long long stride = ipow(4, n - q), n_out = ipow(R1, q) * stride;
    out.assign((size_t)n_out, 0.0);
    long long t = -1;
    for (long long o = 0; o < n_out; ++o) out[(size_t)o] = stage_value(true, t1.data(), (int)R1, tb.fwd[at + (size_t)o], stride, in, &t);
    size_bad += t >= (long long)in.size();
    top_index = t > top_index ? t : top_index;
    at += (size_t)n_out;
    in.swap(out);
  }
  CHECK(size_bad == 0 && top_index < 65536, "n=%d R1=%lld: a forward stage reads index %lld", n, R1, top_index);
  double err = 0.0;
  for (long long mr = 0; mr < M; ++mr) err = std::fmax(err, std::fabs(in[(size_t)mr] - Av[(size_t)tb.rmap[(size_t)mr]]));
  CHECK(err <= 1e-12 * max_abs(Av), "n=%d (%d,%d): forward stages off by %.3e of %.3e", n, S1, K1, err, max_abs(Av));
  in.assign((size_t)M, 0.0);
  for (long long mr = 0; mr < M; ++mr) in[(size_t)mr] = y[(size_t)tb.rmap[(size_t)mr]];
  at = 0;
  size_bad = 0;
  for (int q = n; q >= 1; --q) {
    const long long stride = ipow(4, n - q), n_out = ipow(R1, q - 1) * 4 * stride;
    out.assign((size_t)n_out, 0.0);
    long long t = -1;
    for (long long o = 0; o < n_out; ++o) out[(size_t)o] = stage_value(false, t1.data(), (int)R1, tb.bwd[at + (size_t)o], stride, in, &t);
    size_bad += t >= (long long)in.size();
    top_index = t > top_index ? t : top_index;
    at += (size_t)n_out;
    in.swap(out);
  }
  CHECK(size_bad == 0 && top_index < 65536, "n=%d R1=%lld: a backward stage reads index %lld", n, R1, top_index);
  err = 0.0;
  for (long long j = 0; j < D; ++j) err = std::fmax(err, std::fabs(in[(size_t)j] - ATy[(size_t)j]));
  CHECK(err <= 1e-12 * max_abs(ATy), "n=%d (%d,%d): backward stages off by %.3e of %.3e", n, S1, K1, err, max_abs(ATy));
  // a random table is not paired
  CHECK(!tb.pairedT && tb.last.empty() && tb.try_paired == (n <= 3 && R1 == 6), "n=%d R1=%lld: paired flags of a random table", n, R1);
}

// 'proj-set': three two-outcome settings, rows (1, +-e_a) / 2
void proj_set(double t[24]) {
  memset(t, 0, 24 * sizeof(double));
  for (int r = 0; r < 6; ++r) {
    t[r * 4] = 0.5;
    t[r * 4 + r / 2 + 1] = r % 2 ? -0.5 : 0.5;
  }
}

void check_paired() {
  double t[24], stray[24];
  proj_set(t);
  CHECK(qt::is_paired(t), "is_paired refuses proj-set");
  for (int r = 0; r < 6; ++r)
    for (int k = 1; k < 4; ++k) {
      if (k == r / 2 + 1) continue;
      memcpy(stray, t, sizeof t);
      stray[r * 4 + k] = 1e-300;
      CHECK(!qt::is_paired(stray), "is_paired accepts a stray non-zero at (%d, %d)", r, k);
    }
  // the exact left inverse of proj-set: T^T T = diag(3/2, 1/2, 1/2, 1/2), so pinv(T)^T[r] = (1/3, +-e_a): paired too
  double p1t[24] = {};
  for (int r = 0; r < 6; ++r) {
    p1t[r * 4] = 0.5 / 1.5;
    p1t[r * 4 + r / 2 + 1] = (r % 2 ? -0.5 : 0.5) / 0.5;
  }
  for (int n = 1; n <= 5; ++n) {
    const long long S = ipow(3, n), M = ipow(6, n);
    std::vector<double> ns((size_t)S, 1000.0);
    qt::ProductTables tb;
    CHECK(qt::build_product_tables(n, 3, 2, ns.data(), t, &tb) == qt::TABLES_OK, "proj-set n=%d refused", n);
    CHECK(tb.try_paired == (n <= 3) && tb.pairedT == (n <= 3), "proj-set n=%d: try_paired %d pairedT %d", n, tb.try_paired, tb.pairedT);
    if (n > 3) {
      CHECK(tb.last.empty(), "proj-set n=%d has a `last` table", n);
      continue;
    }
    // `last`: the closed form in0 = 4 r_pre, axis = in0 + a + 1, place = 4 r + a + 1, each in its byte
    CHECK((long long)tb.last.size() == M, "proj-set n=%d: last has %zu entries", n, tb.last.size());
    if ((long long)tb.last.size() != M) continue;
    long long bad = 0;
    for (long long o = 0; o < M; ++o) {
      const int e = tb.last[(size_t)o], rpre = (int)(o / 6), r = (int)(o % 6), a = r / 2;
      const int in0 = e & 0xff, axis = (e >> 8) & 0xff, place = e >> 16;
      bad += !(in0 == 4 * rpre && axis == in0 + a + 1 && place == 4 * r + a + 1 && 4 * rpre + 4 < 256);
    }
    CHECK(bad == 0, "proj-set n=%d: %lld `last` entries off the closed form", n, bad);
    // ... and they evaluate stage n: u_r in[in0] + v_r in[axis] = (row r of T) . in[4 r_pre ..]
    std::vector<double> x((size_t)(M / 6 * 4));
    for (double& z : x) z = uniform01();
    double err = 0.0;
    for (long long o = 0; o < M; ++o) {
      const int e = tb.last[(size_t)o], vi = e >> 16;
      const double got = t[vi] * x[(size_t)((e >> 8) & 0xff)] + t[vi & ~3] * x[(size_t)(e & 0xff)];
      double want = 0.0;
      for (int k = 0; k < 4; ++k) want += t[(o % 6) * 4 + k] * x[(size_t)(o / 6 * 4 + k)];
      err = std::fmax(err, std::fabs(got - want));
    }
    CHECK(err <= 1e-12, "proj-set n=%d: paired stage n off by %.3e", n, err);
    // the image: `last` padded to four entries | T | pinv(T)^T | rinv  (qt::SpecArgs::image)
    const qt::PairedTables pt = qt::classify_paired(tb, p1t);
    CHECK(pt.pairedP, "the exact pinv of proj-set is not paired");
    const size_t nl = (size_t)((M + 3) & ~3LL);
    CHECK(pt.image.size() == nl + 96 + (size_t)M, "proj-set n=%d: image has %zu ints", n, pt.image.size());
    if (pt.image.size() != nl + 96 + (size_t)M) continue;
    bool ok = memcmp(pt.image.data(), tb.last.data(), (size_t)M * sizeof(int)) == 0;
    for (size_t e = (size_t)M; e < nl; ++e) ok = ok && pt.image[e] == 0;
    ok = ok && memcmp(pt.image.data() + nl, t, sizeof t) == 0 && memcmp(pt.image.data() + nl + 48, p1t, sizeof p1t) == 0;
    ok = ok && memcmp(pt.image.data() + nl + 96, tb.rinv.data(), (size_t)M * sizeof(int)) == 0;
    CHECK(ok, "proj-set n=%d: image layout", n);
    for (int r = 0; r < 6; ++r)
      CHECK(pt.cT[2 * r] == t[r * 4] && pt.cT[2 * r + 1] == t[r * 4 + r / 2 + 1] && pt.cP[2 * r] == p1t[r * 4] &&
                pt.cP[2 * r + 1] == p1t[r * 4 + r / 2 + 1], "proj-set n=%d: cT / cP of row %d", n, r);
    // an unpaired pinv: no image
    memcpy(stray, p1t, sizeof stray);
    stray[1 * 4 + 3] = 1e-20;
    const qt::PairedTables pu = qt::classify_paired(tb, stray);
    CHECK(!pu.pairedP && pu.image.empty(), "proj-set n=%d: a stray entry in pinv(T)^T still gives an image", n);
  }
  // 'proj' (one setting of six outcomes): paired, but K = 6^n != 2^n, so no image
  std::vector<double> one(1, 1000.0);
  qt::ProductTables tb;
  double t6[24];
  for (int e = 0; e < 24; ++e) t6[e] = t[e] / 3;
  CHECK(qt::build_product_tables(2, 1, 6, one.data(), t6, &tb) == qt::TABLES_OK && tb.pairedT, "proj n=2");
  CHECK(qt::classify_paired(tb, p1t).pairedP && qt::classify_paired(tb, p1t).image.empty(), "proj n=2: image without K = 2^n");
}

void check_refusals() {
  qt::ProductShape sh;
  CHECK(qt::product_shape(1, 1, 255, &sh) == qt::TABLES_OK && sh.M == 255, "(1, 255) refused");
  CHECK(qt::product_shape(1, 1, 256, &sh) == qt::TABLES_R1 && sh.R1 == 256, "R1 = 256 admitted");
  CHECK(qt::product_shape(1, 16, 16, &sh) == qt::TABLES_R1, "R1 = 16 x 16 admitted");
  CHECK(qt::product_shape(3, 1, 32, &sh) == qt::TABLES_OK && sh.M == 32768, "M = 2^15 refused");
  CHECK(qt::product_shape(1, 1, 32769, &sh) == qt::TABLES_ROWS && sh.M == 32769, "M = 2^15 + 1 admitted");
  CHECK(qt::product_shape(2, 1, 182, &sh) == qt::TABLES_ROWS && sh.M == 182 * 182, "M = 182^2 admitted");
  CHECK(qt::product_shape(5, 46341, 46341, &sh) == qt::TABLES_ROWS && sh.M > 0, "an overflowing shape admitted");
  // the builder refuses the same, and touches neither input
  qt::ProductTables tb;
  CHECK(qt::build_product_tables(1, 1, 32769, nullptr, nullptr, &tb) == qt::TABLES_ROWS && tb.rmap.empty(), "builder: M = 2^15 + 1");
  CHECK(qt::build_product_tables(1, 1, 256, nullptr, nullptr, &tb) == qt::TABLES_R1 && tb.rmap.empty(), "builder: R1 = 256");
}

}  // namespace

int main() {
  const int shapes[4][2] = {{3, 2}, {1, 4}, {1, 6}, {2, 3}};
  for (int n = 1; n <= 5; ++n)
    for (const auto& sk : shapes) check_shape(n, sk[0], sk[1], (n + sk[0]) % 2 == 0);
  // the edges of the admitted range; the last two have M = 2^15 exactly
  check_shape(1, 1, 255, false);
  check_shape(1, 5, 51, false);
  check_shape(2, 1, 181, true);
  check_shape(3, 2, 16, false);
  check_shape(5, 2, 4, false);
  check_paired();
  check_refusals();
  printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

// The index tables of a product POVM (qt_args.h: ProductView), built on the host.  Plain C++: no HIP, no device, so the
// packing below -- the contract with Small::stage_value / Large::stage_value and the paired stage n -- is tested on the
// CPU (tests/host/product_tables_host.cpp).
//
// Arrays of a contraction live in "R-order": index [r_1 .. r_q][k_(q+1) .. k_n], r = s K1 + o the row of the one-qubit
// table T[R1][4], qubit 1 the most significant digit.
//   stage entry  base | sel << 16         out[o] = sum_t tbl(sel, t) in[base + t 4^(n-q)]; forward: row `sel` < R1 of T,
//                                         4 terms; backward: column `sel` < 4, R1 terms
//   `last` entry in0 | axis << 8 | place << 16   stage n of a paired table: u_r in[in0] + v_r in[axis], v_r = T[place]
// A base is below max(R1, 4)^n, a selector below R1, in0 and axis below 4 * 6^(n-1) + 4: the packings hold for
// M = R1^n <= 2^15 rows, R1 <= 255 and n <= 5, and product_shape refuses everything else.
#pragma once
#include <cstring>
#include <vector>

namespace qt {

enum TablesStatus { TABLES_OK = 0, TABLES_ROWS, TABLES_R1 };  // refused: M > 2^15 / R1 > 255

struct ProductShape {
  int n = 0, S1 = 0, K1 = 0;
  long long R1 = 0, S = 0, K = 0, M = 0;  // S1^n settings of K1^n outcomes, M = R1^n rows (saturating at 2^62)
};

// The shape of the n-fold product of an (S1, K1) one-qubit POVM, n = 1 .. 5, S1, K1 >= 1; whether the packings hold it.
inline TablesStatus product_shape(int n, int S1, int K1, ProductShape* sh) {
  auto mul = [](long long a, long long b) { return a > (1LL << 62) / b ? 1LL << 62 : a * b; };
  *sh = ProductShape{n, S1, K1, (long long)S1 * K1, 1, 1, 1};
  for (int q = 0; q < n; ++q) {
    sh->S = mul(sh->S, S1);
    sh->K = mul(sh->K, K1);
    sh->M = mul(sh->M, sh->R1);
  }
  if (sh->M > (1 << 15)) return TABLES_ROWS;
  if (sh->R1 > 255) return TABLES_R1;
  return TABLES_OK;
}

// A six-row table whose rows 2a, 2a+1 are zero outside columns 0 and a+1 (ProductView::pairedT).  tab: [6][4]
inline bool is_paired(const double* tab) {
  for (int r = 0; r < 6; ++r)
    for (int k = 1; k < 4; ++k)
      if (k != r / 2 + 1 && tab[r * 4 + k] != 0.0) return false;
  return true;
}

struct ProductTables {
  ProductShape shape;
  std::vector<double> T;      // [R1][4] the one-qubit table
  std::vector<int> rmap;      // [M] R-order index -> row s K + k of the (S, K) layout
  std::vector<int> rinv;      // [M] the inverse map
  std::vector<double> wrow;   // [M] N_s / sum(N) of each row, R-order
  std::vector<int> fwd, bwd;  // stage 1 .. n / n .. 1 concatenated (Small::fwd_ints / bwd_ints entries)
  std::vector<int> last;      // [M] when pairedT, else empty
  double tot = 0.0, ns_max = 0.0, wuni = 0.0;  // sum and maximum of the shots, ns[0] / tot
  bool uniform = true;        // all shots equal
  bool try_paired = false;    // n <= 3 and R1 = 6: the shape paired stages exist for
  bool pairedT = false;       // ... and T is paired
};

// ns: [S] shots per setting, t1: [R1][4].
inline TablesStatus build_product_tables(int n, int S1, int K1, const double* ns, const double* t1, ProductTables* out) {
  ProductTables& t = *out;
  t = ProductTables{};
  if (TablesStatus st = product_shape(n, S1, K1, &t.shape)) return st;
  const long long R1 = t.shape.R1, S = t.shape.S, K = t.shape.K, M = t.shape.M;
  t.T.assign(t1, t1 + 4 * R1);
  for (long long s = 0; s < S; ++s) {
    t.tot += ns[s];
    if (ns[s] != ns[0]) t.uniform = false;
    if (ns[s] > t.ns_max) t.ns_max = ns[s];
  }
  t.wuni = ns[0] / t.tot;
  t.rmap.resize((size_t)M);
  t.rinv.resize((size_t)M);
  t.wrow.resize((size_t)M);
  for (long long mr = 0; mr < M; ++mr) {  // mr = [r_1 .. r_n], r_q = s_q K1 + o_q
    long long rem = mr, s = 0, o = 0, sp = 1, op = 1;
    for (int q = n - 1; q >= 0; --q) {
      const int r = (int)(rem % R1);
      rem /= R1;
      s += (r / K1) * sp;
      o += (r % K1) * op;
      sp *= S1;
      op *= K1;
    }
    t.rmap[(size_t)mr] = (int)(s * K + o);
    t.rinv[(size_t)(s * K + o)] = (int)mr;
    t.wrow[(size_t)mr] = ns[s] / t.tot;
  }
  auto ipow = [](long long b, int e) {
    long long r = 1;
    for (int i = 0; i < e; ++i) r *= b;
    return r;
  };
  for (int q = 1; q <= n; ++q) {  // forward stage q: out[r_1..r_q][k_(q+1)..k_n]
    const long long Kq = ipow(4, n - q), n_out = ipow(R1, q) * Kq;
    for (long long o = 0; o < n_out; ++o) {
      const long long rpre = o / (R1 * Kq), rq = (o / Kq) % R1, krest = o % Kq;
      t.fwd.push_back((int)((rpre * 4 * Kq + krest) | (rq << 16)));
    }
  }
  for (int q = n; q >= 1; --q) {  // backward stage q: out[r_1..r_(q-1)][k_q..k_n]
    const long long Kq = ipow(4, n - q), n_out = ipow(R1, q - 1) * 4 * Kq;
    for (long long o = 0; o < n_out; ++o) {
      const long long rpre = o / (4 * Kq), kq = (o / Kq) % 4, krest = o % Kq;
      t.bwd.push_back((int)((rpre * R1 * Kq + krest) | (kq << 16)));
    }
  }
  // A paired table at n <= 3: the entries of forward stage n, row by row in R-order (in0 = 4 r_pre, axis = in0 + a + 1,
  // and the place 4 r + a + 1 of v_r in the table).
  t.try_paired = n <= 3 && R1 == 6;
  t.pairedT = t.try_paired && is_paired(t1);
  if (t.pairedT) {
    t.last.resize((size_t)M);
    for (long long o = 0; o < M; ++o) {
      const int rpre = (int)(o / 6), r = (int)(o % 6), a = r / 2;
      t.last[(size_t)o] = (4 * rpre) | (4 * rpre + a + 1) << 8 | (4 * r + a + 1) << 16;
    }
  }
  return TABLES_OK;
}

struct PairedTables {
  bool pairedP = false;           // pinv(T)^T is paired
  double cT[12] = {}, cP[12] = {};  // ProductView::cT / cP: (tab[r][0], tab[r][r / 2 + 1]) of T and pinv(T)^T
  // The table image of the specialised MLE kernels (SpecArgs::image), when both tables are paired and K = 2^n: `last`
  // padded to four entries, T [6][4], pinv(T)^T [6][4] as doubles, rinv [M].  Empty otherwise.
  std::vector<int> image;
};

// For tables with try_paired.  p1t: pinv(T)^T [6][4] as the device computed it -- the values the kernels read, so it is
// classified with no tolerance.
inline PairedTables classify_paired(const ProductTables& t, const double* p1t) {
  PairedTables p;
  p.pairedP = is_paired(p1t);
  for (int r = 0; r < 6; ++r) {
    p.cT[2 * r] = t.T[r * 4];
    p.cT[2 * r + 1] = t.T[r * 4 + r / 2 + 1];
    p.cP[2 * r] = p1t[r * 4];
    p.cP[2 * r + 1] = p1t[r * 4 + r / 2 + 1];
  }
  const long long M = t.shape.M;
  if (t.pairedT && p.pairedP && t.shape.K == (1LL << t.shape.n)) {
    const size_t nl = (size_t)((M + 3) & ~3LL);
    p.image.assign(nl + 2 * 48 + (size_t)M, 0);
    memcpy(p.image.data(), t.last.data(), (size_t)M * sizeof(int));
    memcpy(p.image.data() + nl, t.T.data(), 24 * sizeof(double));
    memcpy(p.image.data() + nl + 48, p1t, 24 * sizeof(double));
    memcpy(p.image.data() + nl + 96, t.rinv.data(), (size_t)M * sizeof(int));
  }
  return p;
}

}  // namespace qt

// affine_map_test -- csrc/affine_map.hpp on inputs where double arithmetic is exact, so every comparison is equality.
// CPU only: includes nothing but that header and links nothing of the library (tests/test_affine_map_cpu.py).
//   affine_map_test                       the built-in cases; prints AFFINE MAP TESTS PASSED
//   affine_map_test <function> <numbers>  evaluates one function on the given arguments and prints the result with 17
//                                         significant digits, for the comparison with the Python restatements:
//     deviation F[6] | inverse F[6] | to_finer F[6] | to_coarser F[6] | corner_displacement A[6] B[6] w h
//     compose_with_inverse F[6] delta[6] w h | increment G[6] d[6] W H | cholesky_solve n A[n*n] rhs[n] (prints "none"
//     for a refusal) | search_separation n1 best msd[n1*n1]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "affine_map.hpp"

using namespace srmap;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static bool same(const AffineMap& A, const AffineMap& B) {
  for (int i = 0; i < 6; ++i)
    if (A.m[i] != B.m[i]) return false;
  return true;
}

// A = L L^T and rhs = A x over the leading n x n block
static void system_of(const int L[6][6], const int* x, int n, double A[6][6], double* rhs) {
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) {
      int s = 0;
      for (int k = 0; k < n; ++k) s += L[i][k] * L[j][k];
      A[i][j] = s;
    }
  }
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += A[i][j] * x[j];
    rhs[i] = s;
  }
}

static void cholesky_cases() {
  // row 2 is (0, 0, 2, ...) and row 5 has 2^2 + 1^2 + 2^2 + 0^2 + 4^2 = 5^2 beside its entry of column 2, so that the
  // sub-system on the indices {2, 5} is [[4, 2], [2, 26]] = [[2, 0], [1, 5]] [[2, 0], [1, 5]]^T
  const int L[6][6] = {{2, 0, 0, 0, 0, 0}, {1, 3, 0, 0, 0, 0}, {0, 0, 2, 0, 0, 0},
                       {2, 1, 1, 1, 0, 0}, {1, 0, 3, 2, 2, 0}, {2, 1, 1, 2, 0, 4}};
  const int x[6] = {3, -2, 5, 1, -4, 2};
  double A[6][6], rhs[6], sol[6];
  system_of(L, x, 6, A, rhs);
  CHECK(cholesky_solve(A, rhs, 6, sol));
  for (int i = 0; i < 6; ++i) CHECK(sol[i] == (double)x[i]);

  // the 2 x 2 sub-system of (tx, ty) as the refinement's LM step forms it: A2 = H[idx][idx], diagonal + lambda * diagonal
  const int idx[2] = {2, 5};
  const double x2[2] = {7.0, -3.0};
  for (int lam = 0; lam < 2; ++lam) {
    double H[6][6];
    if (lam == 0) {
      std::memcpy(H, A, sizeof(H));
    } else {  // diagonal (2, 5) doubles to (4, 10): [[4, 2], [2, 10]] = [[2, 0], [1, 3]] [[2, 0], [1, 3]]^T
      for (auto& row : H) for (double& v : row) v = 0.0;
      H[2][2] = 2.0; H[2][5] = H[5][2] = 2.0; H[5][5] = 5.0;
    }
    const double lambda = (double)lam;
    double A2[6][6], r2[6], s2[6];
    for (int i = 0; i < 2; ++i) {
      for (int j = 0; j < 2; ++j) A2[i][j] = H[idx[i]][idx[j]];
      A2[i][i] = A2[i][i] + lambda * A2[i][i];
    }
    for (int i = 0; i < 2; ++i) r2[i] = A2[i][0] * x2[0] + A2[i][1] * x2[1];
    CHECK(cholesky_solve(A2, r2, 2, s2));
    CHECK(s2[0] == x2[0] && s2[1] == x2[1]);
  }

  // refusals: a zero diagonal entry, a negative one, two equal columns (the pivot of the second is exactly 0)
  double Z[6][6];
  std::memcpy(Z, A, sizeof(Z));
  Z[3][3] = 0.0;
  CHECK(!cholesky_solve(Z, rhs, 6, sol));
  std::memcpy(Z, A, sizeof(Z));
  Z[0][0] = -4.0;
  CHECK(!cholesky_solve(Z, rhs, 6, sol));
  const int Ld[6][6] = {{2, 0, 0, 0, 0, 0}, {1, 3, 0, 0, 0, 0}, {1, 3, 0, 0, 0, 0},
                        {2, 1, 1, 1, 0, 0}, {1, 0, 3, 2, 2, 0}, {2, 1, 1, 2, 0, 4}};
  system_of(Ld, x, 6, Z, rhs);
  for (int i = 0; i < 6; ++i) CHECK(Z[i][1] == Z[i][2]);
  CHECK(!cholesky_solve(Z, rhs, 6, sol));
}

static void map_cases() {
  // unit-determinant linear parts with dyadic entries, translations in multiples of 1/8
  const AffineMap maps[] = {{{1.0, 0.25, 0.375, 0.0, 1.0, -1.125}},
                            {{1.0, 0.0, -2.5, 0.5, 1.0, 0.625}},
                            {{1.5, 0.25, 3.125, 2.0, 1.0, -0.875}},
                            {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}}};
  for (const AffineMap& F : maps) {
    CHECK(same(to_coarser(to_finer(F)), F));
    CHECK(same(inverse(inverse(F)), F));
    CHECK(all_finite(F));
  }
  const AffineMap I = maps[3];
  CHECK(deviation(I) == 0.0);
  CHECK(deviation(maps[0]) == 0.25);
  CHECK(deviation(maps[2]) == 2.0);
  const AffineMap Fi = inverse(maps[0]);  // x = a - 0.25 b - 0.375 - 0.25 * 1.125, y = b + 1.125
  CHECK(same(Fi, AffineMap{{1.0, -0.25, -0.65625, 0.0, 1.0, 1.125}}));
  // a pure translation of (0.375, 0.5) moves every corner by 0.625
  AffineMap T = maps[0];
  T.m[2] += 0.375;
  T.m[5] += 0.5;
  CHECK(corner_displacement(T, maps[0], 9, 17) == 0.625);
  CHECK(corner_displacement(maps[0], maps[0], 9, 17) == 0.0);
  // W = identity: both updates leave the map alone
  const double zero[6] = {0, 0, 0, 0, 0, 0};
  CHECK(same(compose_with_inverse(maps[0], zero, 9, 17), maps[0]));
  CHECK(same(increment(maps[0], zero, 4.0, 8.0), maps[0]));

  AffineMap B = maps[0];
  B.m[4] = std::numeric_limits<double>::quiet_NaN();
  CHECK(!all_finite(B));
  B = maps[0];
  B.m[2] = std::numeric_limits<double>::infinity();
  CHECK(!all_finite(B));
  B.m[2] = -std::numeric_limits<double>::infinity();
  CHECK(!all_finite(B));
}

static void separation_cases() {
  // one clear minimum: 1 at the centre of a 5 x 5 table of 4s
  std::vector<double> t(25, 4.0);
  t[12] = 1.0;
  CHECK(search_separation(t.data(), 5, 12) == 0.75);
  // a runner-up inside the 3 x 3 exclusion zone is ignored: 2 next to the minimum, 8 as the smallest entry outside
  std::fill(t.begin(), t.end(), 8.0);
  t[12] = 1.0;
  t[13] = 2.0;
  t[6] = 2.0;
  CHECK(search_separation(t.data(), 5, 12) == 0.875);
  // entries of -1 (candidates that were not evaluated) are skipped
  t[0] = -1.0;
  t[24] = -1.0;
  t[4] = 2.0;
  CHECK(search_separation(t.data(), 5, 12) == 0.5);
  // no runner-up at all, or a runner-up of 0: separation 0
  std::fill(t.begin(), t.end(), -1.0);
  t[12] = 1.0;
  CHECK(search_separation(t.data(), 5, 12) == 0.0);
  std::fill(t.begin(), t.end(), 0.0);
  CHECK(search_separation(t.data(), 5, 12) == 0.0);
}

static void print(const double* v, int n) {
  for (int i = 0; i < n; ++i) std::printf("%s%.17g", i ? " " : "", v[i]);
  std::printf("\n");
}

static int evaluate(int argc, char** argv) {
  const char* fn = argv[1];
  std::vector<double> a;
  for (int i = 2; i < argc; ++i) a.push_back(std::strtod(argv[i], nullptr));
  auto need = [&](size_t n) {
    if (a.size() != n) {
      std::fprintf(stderr, "%s: expected %zu numbers, got %zu\n", fn, n, a.size());
      std::exit(2);
    }
  };
  auto map_at = [&](size_t i) {
    AffineMap M;
    for (int k = 0; k < 6; ++k) M.m[k] = a[i + k];
    return M;
  };
  if (!std::strcmp(fn, "deviation")) {
    need(6);
    const double d = deviation(map_at(0));
    print(&d, 1);
  } else if (!std::strcmp(fn, "inverse")) {
    need(6);
    print(inverse(map_at(0)).m, 6);
  } else if (!std::strcmp(fn, "to_finer")) {
    need(6);
    print(to_finer(map_at(0)).m, 6);
  } else if (!std::strcmp(fn, "to_coarser")) {
    need(6);
    print(to_coarser(map_at(0)).m, 6);
  } else if (!std::strcmp(fn, "corner_displacement")) {
    need(14);
    const double d = corner_displacement(map_at(0), map_at(6), (int)a[12], (int)a[13]);
    print(&d, 1);
  } else if (!std::strcmp(fn, "compose_with_inverse")) {
    need(14);
    print(compose_with_inverse(map_at(0), &a[6], (int)a[12], (int)a[13]).m, 6);
  } else if (!std::strcmp(fn, "increment")) {
    need(14);  // the centre as motion_refinement.hip forms it
    print(increment(map_at(0), &a[6], 0.5 * (double)((int)a[12] - 1), 0.5 * (double)((int)a[13] - 1)).m, 6);
  } else if (!std::strcmp(fn, "cholesky_solve")) {
    const int n = a.empty() ? 0 : (int)a[0];
    if (n < 1 || n > 6) return 2;
    need(1 + (size_t)n * n + n);
    double A[6][6] = {}, x[6];
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) A[i][j] = a[1 + i * n + j];
    if (cholesky_solve(A, &a[1 + n * n], n, x)) print(x, n);
    else std::printf("none\n");
  } else if (!std::strcmp(fn, "search_separation")) {
    const int n1 = a.empty() ? 0 : (int)a[0];
    if (n1 < 1) return 2;
    need(2 + (size_t)n1 * n1);
    const double s = search_separation(&a[2], n1, (int)a[1]);
    print(&s, 1);
  } else {
    std::fprintf(stderr, "unknown function %s\n", fn);
    return 2;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return evaluate(argc, argv);
  cholesky_cases();
  map_cases();
  separation_cases();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("AFFINE MAP TESTS PASSED\n");
  return 0;
}

// geom_common_test.cpp -- the shared pieces of the geometry solvers (xfeatslam_amd/csrc/geom_common.h) against the obvious forms, on the host,
// under AddressSanitizer + UBSan; compiled from the header alone.  geo_set<K> against the std::vector swap-remove it stands for, the two
// instances of geo_jacobi (rows cached / rows at run time) against each other by bits, the orthogonality of the result, a matrix of NaNs, the tie
// rules of geo_min_col and geo_order3, and the one-liners.  Exit code 0 = clean.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "geom_common.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "geom_common_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0 * 2.0 - 1.0; }     // -1 .. 1

// ---- the minimal set: vAvailableIndices as the reference keeps it -------------------------------------------------------------------------------------
static int random_int(int draw, int rand_max, int d) {                     // RandomInt(0, d - 1), a draw outside 0 .. rand_max clamped into the vector
    const double v = ((double)draw / ((double)rand_max + 1.0)) * (double)d;
    if (v < 0.0) return 0;
    return v >= (double)d ? d - 1 : (int)v;
}
template <int K>
static int set_case(const int* draws, int rand_max, int N) {
    std::vector<int> avail(N);
    for (int i = 0; i < N; ++i) avail[i] = i;
    int want[K], got[K];
    for (int j = 0; j < K; ++j) {
        const int r = random_int(draws[j], rand_max, (int)avail.size());
        want[j] = avail[r];
        avail[r] = avail.back();
        avail.pop_back();
    }
    geo_set<K>(draws, rand_max, N, got);
    for (int j = 0; j < K; ++j) CHECK(got[j] == want[j]);
    for (int j = 0; j < K; ++j)
        for (int i = 0; i < j; ++i) CHECK(got[i] != got[j] && got[j] >= 0 && got[j] < N);
    return 0;
}
template <int K>
static int set_cases() {
    const int rand_maxes[2] = {32767, INT_MAX};
    for (int rm = 0; rm < 2; ++rm) {
        const int rand_max = rand_maxes[rm];
        const int special[8] = {0, rand_max, -1, -5, INT_MIN, INT_MAX, rand_max / 2, 40000};        // the two ends, and values outside 0 .. rand_max
        const int Ns[5] = {K, K + 1, K + 2, K + 3, 1000};
        for (int n = 0; n < 5; ++n) {
            int d[K];
            for (int s = 0; s < 8; ++s) {                                   // the same draw K times: every removal hits the front, the back or a clamped end
                for (int j = 0; j < K; ++j) d[j] = special[s];
                if (set_case<K>(d, rand_max, Ns[n])) return 1;
            }
            for (int rep = 0; rep < 400; ++rep) {                           // any mixture, a special value at every third place on average
                for (int j = 0; j < K; ++j) d[j] = rnd() % 3 == 0 ? special[rnd() % 8] : (int)(rnd() % ((u64)rand_max + 1));
                if (set_case<K>(d, rand_max, Ns[n])) return 1;
            }
        }
    }
    return 0;
}

// ---- the Jacobi: cached rows against run-time rows ---------------------------------------------------------------------------------------------------
// A: rows x N, row-major.  The run-time instance works in storage of stride 3, the cached one of stride 1: the same numbers to the bit.
template <int M>
static int jacobi_case(const double* A, int N, bool expect_rotations) {
    const int SR = 3;
    std::vector<double> u1(M * N), v1(N * N), u0((size_t)M * N * SR, 7.0), v0((size_t)N * N * SR, 7.0);
    const GeoMat U1{u1.data(), 1}, V1{v1.data(), 1}, U0{u0.data(), SR}, V0{v0.data(), SR};
    for (int k = 0; k < M * N; ++k) { U1(k) = A[k]; U0(k) = A[k]; }
    const int r1 = geo_jacobi<M>(U1, V1, N), r0 = geo_jacobi<0>(U0, V0, N, M);
    CHECK(r1 == r0 && (r1 > 0) == expect_rotations);
    for (int k = 0; k < M * N; ++k) CHECK(memcmp(&U1(k), &U0(k), 8) == 0);
    for (int k = 0; k < N * N; ++k) CHECK(memcmp(&V1(k), &V0(k), 8) == 0);
    for (size_t k = 0; k < u0.size(); ++k) if (k % SR) CHECK(u0[k] == 7.0);       // nothing between the elements was touched
    for (size_t k = 0; k < v0.size(); ++k) if (k % SR) CHECK(v0[k] == 7.0);
    if (!expect_rotations) {                                                // a NaN rotates nothing: U as given, V the identity
        for (int k = 0; k < M * N; ++k) CHECK(memcmp(&U1(k), &A[k], 8) == 0);
        for (int k = 0; k < N * N; ++k) CHECK(V1(k) == (k / N == k % N ? 1.0 : 0.0));
        return 0;
    }
    for (int a = 0; a < N; ++a)
        for (int b = a + 1; b < N; ++b) {
            const double d = geo_col_dot(U1, M, N, a, b), na = geo_col_dot(U1, M, N, a, a), nb = geo_col_dot(U1, M, N, b, b);
            CHECK(std::fabs(d) <= 1e-12 * std::sqrt(na) * std::sqrt(nb));
        }
    for (int a = 0; a < N; ++a)                                             // V stayed orthogonal, and U = A V
        for (int b = 0; b < N; ++b) {
            const double d = geo_col_dot(V1, N, N, a, b);
            CHECK(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-12);
        }
    for (int r = 0; r < M; ++r)
        for (int c = 0; c < N; ++c) {
            double s = 0.0, mag = 0.0;
            for (int k = 0; k < N; ++k) { s += A[r * N + k] * V1(k * N + c); mag += std::fabs(A[r * N + k]); }
            CHECK(std::fabs(s - U1(r * N + c)) <= 1e-12 * (mag + 1.0));
        }
    return 0;
}
template <int N>
static int jacobi_symmetric(int reps) {
    double A[N * N];
    for (int rep = 0; rep < reps; ++rep) {
        for (int r = 0; r < N; ++r)
            for (int c = r; c < N; ++c) { const double v = uni() * (rep % 2 ? 1e3 : 1.0); A[r * N + c] = v; A[c * N + r] = v; }
        if (jacobi_case<N>(A, N, true)) return 1;
    }
    for (int k = 0; k < N * N; ++k) A[k] = std::numeric_limits<double>::quiet_NaN();
    return jacobi_case<N>(A, N, false);
}

int main() {
    if (set_cases<3>() || set_cases<6>() || set_cases<8>()) return 1;
    CHECK(geo_draw_index(0, 32767, 5) == 0 && geo_draw_index(32767, 32767, 5) == 4 && geo_draw_index(-1, 32767, 5) == 0 && geo_draw_index(40000, 32767, 5) == 4);

    if (jacobi_symmetric<3>(50) || jacobi_symmetric<9>(50) || jacobi_symmetric<12>(50)) return 1;
    double A[16 * 9];
    for (int rep = 0; rep < 50; ++rep) {
        for (int k = 0; k < 16 * 9; ++k) A[k] = uni();
        if (jacobi_case<16>(A, 9, true)) return 1;
    }
    for (int k = 0; k < 16 * 9; ++k) A[k] = std::numeric_limits<double>::quiet_NaN();
    if (jacobi_case<16>(A, 9, false)) return 1;

    // the tie rules on equal norms: first / last least column, order3 stable
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double m[9], n2[3]; int o[3];
    const GeoMat Mx{m, 1};
    auto diag = [&](double a, double b, double c) { for (int k = 0; k < 9; ++k) m[k] = 0.0; m[0] = a; m[4] = b; m[8] = c; };
    diag(2.0, 2.0, 2.0);
    CHECK(geo_min_col(Mx, 3, 3, false) == 0 && geo_min_col(Mx, 3, 3, true) == 2);
    geo_order3(Mx, o, n2);
    CHECK(o[0] == 0 && o[1] == 1 && o[2] == 2 && n2[0] == 4.0 && n2[1] == 4.0 && n2[2] == 4.0);
    diag(1.0, 2.0, 1.0);
    CHECK(geo_min_col(Mx, 3, 3, false) == 0 && geo_min_col(Mx, 3, 3, true) == 2);
    geo_order3(Mx, o, n2);
    CHECK(o[0] == 1 && o[1] == 0 && o[2] == 2);
    diag(2.0, 1.0, 1.0);
    CHECK(geo_min_col(Mx, 3, 3, false) == 1 && geo_min_col(Mx, 3, 3, true) == 2);
    geo_order3(Mx, o, n2);
    CHECK(o[0] == 0 && o[1] == 1 && o[2] == 2);
    diag(1.0, 2.0, 2.0);
    geo_order3(Mx, o, n2);
    CHECK(o[0] == 1 && o[1] == 2 && o[2] == 0);
    diag(2.0, nan, 2.0);                                                    // a NaN behind column 0 never wins
    CHECK(geo_min_col(Mx, 3, 3, false) == 0 && geo_min_col(Mx, 3, 3, true) == 2);

    const float Af[9] = {2.0f, 0.0f, 1.0f, 1.0f, 3.0f, 0.0f, 0.0f, 1.0f, 4.0f};
    const double Ad[9] = {2.0, 0.0, 1.0, 1.0, 3.0, 0.0, 0.0, 1.0, 4.0};
    CHECK(geo_det3(Af) == 25.0f && geo_det3(Ad) == 25.0);
    CHECK(geo_clamp_its(0, 10) == 1 && geo_clamp_its(INT_MIN, 10) == 1 && geo_clamp_its(7, 10) == 7 && geo_clamp_its(INT_MAX, 10) == 10);
    CHECK(geo_al16(0) == 0 && geo_al16(1) == 16 && geo_al16(16) == 16 && geo_al16(17) == 32);
    float s[GEO_LANES];
    for (int l = 0; l < GEO_LANES; ++l) s[l] = (float)l;
    CHECK(geo_tree_fold(s) == 32640.0f);
    printf("geom_common_test ok\n");
    return 0;
}

// capi_mlpnp.cpp -- the entry points of include/xfeat_hip.h behind MLPnPsolver in Tracking::Relocalization (xfh_mlpnp_*): the pieces of the rule on
// the host (mlpnp_math.h, the kernels' own lines), the whole rule on one host thread, the device form and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "mlpnp_math.h"
#include <math.h>
#include <vector>

#define ML_MAX_POINTS (1 << 24)

static bool ml_dims_ok(int B, int n, int nq, int max_iters) {
    return B >= 1 && B <= 65535 && n >= 1 && n <= XFH_GRID_MAX_N && nq >= 1 && nq <= ML_MAX_POINTS && max_iters >= 1 && max_iters <= ML_MAX_ITERS;
}
static bool ml_scalars_ok(const xfh_camera* cam, float max_err, int chunk, int rand_max) { return cam && isfinite(max_err) && chunk >= 0 && rand_max >= 1; }
static bool ml_stride_ok(int B, int max_iters, size_t draws_stride) { return draws_stride == 0 || draws_stride >= (size_t)max_iters * ML_MIN_SET || B == 1; }

static MlArgs ml_args(int B, int n, int nq, const float* xy_un, const int* assigned, const float* points, const uint8_t* valid, const xfh_camera* cam, float max_err,
                      int min_matches, const int* n_matches, const int* iters_of_N, const int* min_of_N, int chunk, const int* start_iter, int max_iters,
                      const int* draws, size_t draws_stride, int rand_max, void* ws, int* header, float* Tcw, uint8_t* inliers, int* assigned_out) {
    MlArgs a = {};
    a.B = B; a.n = n; a.nq = nq; a.max_iters = max_iters; a.rand_max = rand_max; a.min_matches = min_matches; a.chunk = chunk; a.draws_stride = draws_stride;
    a.cam = GeoCam{cam->fx, cam->fy, cam->cx, cam->cy}; a.max_err = max_err; a.xy_un = xy_un; a.points = points; a.assigned = assigned; a.n_matches = n_matches;
    a.iters_of_N = iters_of_N; a.min_of_N = min_of_N; a.start_iter = start_iter; a.draws = draws; a.valid = valid; a.ws = (unsigned char*)ws; a.header = header;
    a.Tcw = Tcw; a.inliers = inliers; a.assigned_out = assigned_out;
    return a;
}

extern "C" {

size_t xfh_mlpnp_workspace_bytes(int n, int nq, int B, int max_iters) {
    if (!ml_dims_ok(B, n, nq, max_iters)) return 0;
    return ml_layout(n, max_iters).per_problem * (size_t)B;
}

int xfh_mlpnp_iterations_table(double prob, int min_inliers, int max_its, int min_set, float eps, int n, int* iters_of_N, int* min_inliers_of_N) {
    if (!iters_of_N || !min_inliers_of_N || n < 0 || n > XFH_GRID_MAX_N || min_set != ML_MIN_SET || !(eps >= 0.0f && eps <= 1.0f) || min_inliers < 0) return XFH_ERR_INVALID_ARG;
    for (int N = 0; N <= n; ++N) ml_params(prob, min_inliers, max_its, min_set, eps, N, iters_of_N + N, min_inliers_of_N + N);
    return XFH_OK;
}

int xfh_mlpnp_set(const int* draws6, int rand_max, int N, int* set6) {
    if (!draws6 || !set6 || rand_max < 1 || N < ML_MIN_SET) return XFH_ERR_INVALID_ARG;
    geo_set<ML_MIN_SET>(draws6, rand_max, N, set6);
    return XFH_OK;
}

int xfh_mlpnp_nullspace(const double* f, double* rs) {
    if (!f || !rs) return XFH_ERR_INVALID_ARG;
    ml_nullspace(f, rs);
    return XFH_OK;
}

int xfh_mlpnp_compute_pose(int m, const float* f, const float* p, const uint8_t* use_or_null, int fold, double* Rt, int* planar) {
    if (m < ML_MIN_SET || m > XFH_GRID_MAX_N || !f || !p || !Rt || !planar) return XFH_ERR_INVALID_ARG;
    std::vector<double> rs((size_t)m * 6);
    for (int c = 0; c < m; ++c) {
        const double fd[3] = {(double)f[3 * (size_t)c], (double)f[3 * (size_t)c + 1], (double)f[3 * (size_t)c + 2]};
        ml_nullspace(fd, rs.data() + 6 * (size_t)c);
    }
    return ml_host_pose(m, f, p, rs.data(), use_or_null, fold != 0, Rt, planar) ? XFH_OK : XFH_ERR_INVALID_ARG;      // fewer than six points in use
}

int xfh_mlpnp_check(const double* Rt, const xfh_camera* cam, const float* X, const float* xy, float max_err, float* error2, int* inlier) {
    if (!Rt || !cam || !X || !xy || !error2 || !inlier) return XFH_ERR_INVALID_ARG;
    *inlier = ml_check(Rt, GeoCam{cam->fx, cam->fy, cam->cx, cam->cy}, X, xy, max_err, error2);
    return XFH_OK;
}

int xfh_mlpnp_solve_host(int B, int n, int nq, const float* xy_un, const int* assigned, const float* points, const uint8_t* point_valid_or_null,
                         const xfh_camera* cam, float max_err, int min_matches, const int* n_matches_or_null, const int* iters_of_N,
                         const int* min_inliers_of_N, int chunk, const int* start_iter_or_null, int max_iters, const int* draws,
                         size_t draws_problem_stride, int rand_max, void* workspace, int* header, float* Tcw, uint8_t* inliers, int* assigned_out) {
    if (!ml_dims_ok(B, n, nq, max_iters) || !ml_scalars_ok(cam, max_err, chunk, rand_max) || !ml_stride_ok(B, max_iters, draws_problem_stride)) return XFH_ERR_INVALID_ARG;
    if (!xy_un || !assigned || !points || !iters_of_N || !min_inliers_of_N || !draws || !workspace || !header || !Tcw || !inliers || !assigned_out) return XFH_ERR_INVALID_ARG;
    if (misaligned(3, xy_un, assigned, points, n_matches_or_null, iters_of_N, min_inliers_of_N, start_iter_or_null, draws, header, Tcw, assigned_out) ||
        misaligned(15, workspace)) return XFH_ERR_INVALID_ARG;
    const MlArgs a = ml_args(B, n, nq, xy_un, assigned, points, point_valid_or_null, cam, max_err, min_matches, n_matches_or_null, iters_of_N, min_inliers_of_N, chunk,
                             start_iter_or_null, max_iters, draws, draws_problem_stride, rand_max, workspace, header, Tcw, inliers, assigned_out);
    std::vector<unsigned char> flag((size_t)n);
    for (int b = 0; b < B; ++b) ml_host_problem(a, b, flag.data());
    return XFH_OK;
}

int xfh_mlpnp_solve_device(xfh_ctx* c, int B, int n, int nq, const float* d_xy_un, const int* d_assigned, const float* d_points,
                           const uint8_t* d_point_valid_or_null, const xfh_camera* cam, float max_err, int min_matches, const int* d_n_matches_or_null,
                           const int* d_iters_of_N, const int* d_min_inliers_of_N, int chunk, const int* d_start_iter_or_null, int max_iters,
                           const int* d_draws, size_t draws_problem_stride, int rand_max, void* d_workspace, int* d_header, float* d_Tcw,
                           uint8_t* d_inliers, int* d_assigned_out) {
    if (!c || !ml_dims_ok(B, n, nq, max_iters) || !ml_scalars_ok(cam, max_err, chunk, rand_max) || !ml_stride_ok(B, max_iters, draws_problem_stride))
        return XFH_ERR_INVALID_ARG;
    if (!d_xy_un || !d_assigned || !d_points || !d_iters_of_N || !d_min_inliers_of_N || !d_draws || !d_workspace || !d_header || !d_Tcw || !d_inliers ||
        !d_assigned_out) return XFH_ERR_INVALID_ARG;
    if (misaligned(3, d_xy_un, d_assigned, d_points, d_n_matches_or_null, d_iters_of_N, d_min_inliers_of_N, d_start_iter_or_null, d_draws, d_header, d_Tcw,
                   d_assigned_out) || misaligned(15, d_workspace)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const MlArgs a = ml_args(B, n, nq, d_xy_un, d_assigned, d_points, d_point_valid_or_null, cam, max_err, min_matches, d_n_matches_or_null, d_iters_of_N,
                             d_min_inliers_of_N, chunk, d_start_iter_or_null, max_iters, d_draws, draws_problem_stride, rand_max, d_workspace, d_header, d_Tcw,
                             d_inliers, d_assigned_out);
    HIPCK(c, launch_mlpnp_solve(c, a));
    return XFH_OK;
}

int xfh_mlpnp_solve(xfh_ctx* c, int n, int nq, const float* xy_un, const int* assigned, const float* points, const uint8_t* point_valid_or_null,
                    const xfh_camera* cam, float max_err, const int* iters_of_N, const int* min_inliers_of_N, int chunk, int start_iter, int max_iters,
                    const int* draws, int rand_max, int* header, float* Tcw, uint8_t* inliers, int* assigned_out) {
    if (!c || !ml_dims_ok(1, n, nq, max_iters) || !ml_scalars_ok(cam, max_err, chunk, rand_max)) return XFH_ERR_INVALID_ARG;
    if (!xy_un || !assigned || !points || !iters_of_N || !min_inliers_of_N || !draws || !header || !Tcw || !inliers || !assigned_out) return XFH_ERR_INVALID_ARG;
    const size_t N1 = (size_t)n;
    HostStage s{c};
    auto xy = s.in<float>(xy_un, N1 * 8); auto as = s.in<int>(assigned, N1 * 4); auto pt = s.in<float>(points, (size_t)nq * 12);
    auto va = s.in_opt<uint8_t>(point_valid_or_null, (size_t)nq); auto ti = s.in<int>(iters_of_N, (N1 + 1) * 4); auto tm = s.in<int>(min_inliers_of_N, (N1 + 1) * 4);
    auto st = s.in<int>(&start_iter, 4); auto dr = s.in<int>(draws, (size_t)max_iters * ML_MIN_SET * 4);
    auto ws = s.tmp<unsigned char>(xfh_mlpnp_workspace_bytes(n, nq, 1, max_iters));
    auto oh = s.out<int>(header, ML_HEADER_INTS * 4); auto oT = s.out<float>(Tcw, 48); auto oi = s.out<uint8_t>(inliers, N1); auto oa = s.out<int>(assigned_out, N1 * 4);
    // a call that reports no pose leaves Tcw, and one with too few correspondences everything but the header, as it was: the caller's arrays go up
    // first so that they come back unchanged
    for (int i = oT.i; i < s.n; ++i) s.pc[i].src = s.pc[i].dst;
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_mlpnp_solve_device(c, 1, n, nq, xy, as, pt, va, cam, max_err, 0, nullptr, ti, tm, chunk, st, max_iters, dr, 0, rand_max, (unsigned char*)ws, oh,
                                          oT, oi, oa);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"

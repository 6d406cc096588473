// capi_sim3solve.cpp -- the entry points of include/xfeat_hip.h behind Sim3Solver and the merge in front of it in
// LoopClosing::DetectCommonRegionsFromBoW (xfh_sim3_solve*, xfh_sim3_merge_matches*): the pieces of the rule on the host (sim3solve_math.h, the
// kernels' own lines), the whole rule on one host thread, the device forms and the host-pointer forms (host_stage.h).
#include "host_stage.h"
#include "sim3solve_math.h"
#include <math.h>
#include <vector>

#define S3_MAX_POINTS (1 << 24)

static bool s3_dims_ok(int B, int n1, int M) { return B >= 1 && B <= 65535 && n1 >= 1 && n1 <= XFH_GRID_MAX_N && M >= 1 && M <= S3_MAX_POINTS; }
static bool s3_scalars_ok(const xfh_camera* cam1, const xfh_camera* cam2, float max_err1, float max_err2, int min_inliers, int max_iters, int rand_max) {
    return cam1 && cam2 && isfinite(max_err1) && isfinite(max_err2) && min_inliers >= 0 && max_iters >= 1 && max_iters <= S3_MAX_ITERS && rand_max >= 1;
}
static bool s3_strides_ok(int B, int max_iters, size_t draws_stride, size_t T1w_stride) {
    return (draws_stride == 0 || draws_stride >= (size_t)max_iters * 3 || B == 1) && (T1w_stride == 0 || T1w_stride >= 12 || B == 1);
}
static bool s3_merge_dims_ok(int J, int n1, int n2, int M) {
    return J >= 1 && J <= 65535 && n1 >= 1 && n1 <= XFH_GRID_MAX_N && n2 >= 1 && n2 <= XFH_GRID_MAX_N && M >= 1 && M <= S3_MAX_POINTS;
}
static GeoCam s3_cam(const xfh_camera* c) { return GeoCam{c->fx, c->fy, c->cx, c->cy}; }

static S3Args s3_args(int B, int n1, int M, const float* points, const int* point1, const int* matched, const float* T1w, size_t T1w_stride, const float* T2w,
                      const xfh_camera* cam1, const xfh_camera* cam2, float max_err1, float max_err2, int fix_scale, int min_inliers, int min_matches,
                      const int* num_matches, const int* iters_of_N, int max_iters, const int* draws, size_t draws_stride, int rand_max, void* ws,
                      int* header, float* floats, uint8_t* inliers, float* Tcw, float* Ow) {
    S3Args a = {};
    a.B = B; a.n1 = n1; a.M = M; a.max_iters = max_iters; a.rand_max = rand_max; a.min_inliers = min_inliers; a.min_matches = min_matches; a.fix_scale = fix_scale;
    a.draws_stride = draws_stride; a.T1w_stride = T1w_stride; a.cam1 = s3_cam(cam1); a.cam2 = s3_cam(cam2); a.max_err1 = max_err1; a.max_err2 = max_err2;
    a.points = points; a.T1w = T1w; a.T2w = T2w; a.point1 = point1; a.matched = matched; a.num_matches = num_matches; a.iters_of_N = iters_of_N; a.draws = draws;
    a.ws = (unsigned char*)ws; a.header = header; a.fout = floats; a.inliers = inliers; a.Tcw = Tcw; a.Ow = Ow;
    return a;
}

extern "C" {

size_t xfh_sim3_solve_workspace_bytes(int n1, int M, int B) {
    if (!s3_dims_ok(B, n1, M)) return 0;
    return s3_workspace_bytes(n1, M, B);
}

int xfh_sim3_solve_iterations(double prob, int min_inliers, int max_its, int N) { return s3_iterations(prob, min_inliers, max_its, N); }

int xfh_sim3_solve_iterations_table(double prob, int min_inliers, int max_its, int n1, int* iters_of_N) {
    if (!iters_of_N || n1 < 0) return XFH_ERR_INVALID_ARG;
    for (int N = 0; N <= n1; ++N) iters_of_N[N] = s3_iterations(prob, min_inliers, max_its, N);
    return XFH_OK;
}

int xfh_sim3_solve_set(const int* draws3, int rand_max, int N, int* set3) {
    if (!draws3 || !set3 || rand_max < 1 || N < 3) return XFH_ERR_INVALID_ARG;
    geo_set<3>(draws3, rand_max, N, set3);
    return XFH_OK;
}

int xfh_sim3_solve_horn(const float* P1, const float* P2, int fix_scale, float* hyp) {
    if (!P1 || !P2 || !hyp) return XFH_ERR_INVALID_ARG;
    s3_horn(P1, P2, fix_scale != 0, hyp);
    return XFH_OK;
}

int xfh_sim3_solve_check(const float* T12, const float* T21, const xfh_camera* cam1, const xfh_camera* cam2, const float* X1, const float* X2, float max_err1,
                         float max_err2, float* err, int* inlier) {
    if (!T12 || !T21 || !cam1 || !cam2 || !X1 || !X2 || !err || !inlier) return XFH_ERR_INVALID_ARG;
    float p1[2], p2[2];
    const GeoCam k1 = s3_cam(cam1), k2 = s3_cam(cam2);
    s3_project(k1, X1, p1); s3_project(k2, X2, p2);
    *inlier = s3_check(T12, T21, k1, k2, X1, X2, p1, p2, max_err1, max_err2, err);
    return XFH_OK;
}

int xfh_sim3_solve_host(int B, int n1, int M, const float* points, const int* point1, const int* matched, const float* T1w, size_t T1w_problem_stride,
                        const float* T2w, const xfh_camera* cam1, const xfh_camera* cam2, float max_err1, float max_err2, int fix_scale, int min_inliers,
                        int min_matches, const int* num_matches_or_null, const int* iters_of_N, int max_iters, const int* draws, size_t draws_problem_stride,
                        int rand_max, void* workspace, int* header, float* floats, uint8_t* inliers, float* Tcw, float* Ow) {
    if (!s3_dims_ok(B, n1, M) || !s3_scalars_ok(cam1, cam2, max_err1, max_err2, min_inliers, max_iters, rand_max) ||
        !s3_strides_ok(B, max_iters, draws_problem_stride, T1w_problem_stride)) return XFH_ERR_INVALID_ARG;
    if (!points || !point1 || !matched || !T1w || !T2w || !iters_of_N || !draws || !workspace || !header || !floats || !inliers || !Tcw || !Ow) return XFH_ERR_INVALID_ARG;
    if (misaligned(3, points, point1, matched, T1w, T2w, num_matches_or_null, iters_of_N, draws, header, floats, Tcw, Ow) || misaligned(15, workspace))
        return XFH_ERR_INVALID_ARG;
    const S3Args a = s3_args(B, n1, M, points, point1, matched, T1w, T1w_problem_stride, T2w, cam1, cam2, max_err1, max_err2, fix_scale, min_inliers, min_matches,
                             num_matches_or_null, iters_of_N, max_iters, draws, draws_problem_stride, rand_max, workspace, header, floats, inliers, Tcw, Ow);
    for (int b = 0; b < B; ++b) s3_host_problem(a, b);
    return XFH_OK;
}

int xfh_sim3_solve_device(xfh_ctx* c, int B, int n1, int M, const float* d_points, const int* d_point1, const int* d_matched, const float* d_T1w,
                          size_t T1w_problem_stride, const float* d_T2w, const xfh_camera* cam1, const xfh_camera* cam2, float max_err1, float max_err2,
                          int fix_scale, int min_inliers, int min_matches, const int* d_num_matches_or_null, const int* d_iters_of_N, int max_iters,
                          const int* d_draws, size_t draws_problem_stride, int rand_max, void* d_workspace, int* d_header, float* d_floats, uint8_t* d_inliers,
                          float* d_Tcw, float* d_Ow) {
    if (!c || !s3_dims_ok(B, n1, M) || !s3_scalars_ok(cam1, cam2, max_err1, max_err2, min_inliers, max_iters, rand_max) ||
        !s3_strides_ok(B, max_iters, draws_problem_stride, T1w_problem_stride)) return XFH_ERR_INVALID_ARG;
    if (!d_points || !d_point1 || !d_matched || !d_T1w || !d_T2w || !d_iters_of_N || !d_draws || !d_workspace || !d_header || !d_floats || !d_inliers || !d_Tcw ||
        !d_Ow) return XFH_ERR_INVALID_ARG;
    if (misaligned(3, d_points, d_point1, d_matched, d_T1w, d_T2w, d_num_matches_or_null, d_iters_of_N, d_draws, d_header, d_floats, d_Tcw, d_Ow) ||
        misaligned(15, d_workspace)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const S3Args a = s3_args(B, n1, M, d_points, d_point1, d_matched, d_T1w, T1w_problem_stride, d_T2w, cam1, cam2, max_err1, max_err2, fix_scale, min_inliers,
                             min_matches, d_num_matches_or_null, d_iters_of_N, max_iters, d_draws, draws_problem_stride, rand_max, d_workspace, d_header, d_floats,
                             d_inliers, d_Tcw, d_Ow);
    HIPCK(c, launch_sim3_solve(c, a));
    return XFH_OK;
}

int xfh_sim3_solve(xfh_ctx* c, int n1, int M, const float* points, const int* point1, const int* matched, const float* T1w, const float* T2w,
                   const xfh_camera* cam1, const xfh_camera* cam2, float max_err1, float max_err2, int fix_scale, int min_inliers, const int* iters_of_N,
                   int max_iters, const int* draws, int rand_max, int* header, float* floats, uint8_t* inliers, float* Tcw, float* Ow) {
    if (!c || !s3_dims_ok(1, n1, M) || !s3_scalars_ok(cam1, cam2, max_err1, max_err2, min_inliers, max_iters, rand_max)) return XFH_ERR_INVALID_ARG;
    if (!points || !point1 || !matched || !T1w || !T2w || !iters_of_N || !draws || !header || !floats || !inliers || !Tcw || !Ow) return XFH_ERR_INVALID_ARG;
    const size_t N1 = (size_t)n1;
    HostStage s{c};
    auto pt = s.in<float>(points, (size_t)M * 12); auto p1 = s.in<int>(point1, N1 * 4); auto mt = s.in<int>(matched, N1 * 4); auto t1 = s.in<float>(T1w, 48);
    auto t2 = s.in<float>(T2w, 48); auto tb = s.in<int>(iters_of_N, (N1 + 1) * 4); auto dr = s.in<int>(draws, (size_t)max_iters * 12);
    auto ws = s.tmp<unsigned char>(xfh_sim3_solve_workspace_bytes(n1, M, 1));
    auto oh = s.out<int>(header, S3_HEADER_INTS * 4); auto of = s.out<float>(floats, S3_FLOATS * 4); auto oi = s.out<uint8_t>(inliers, N1);
    auto oT = s.out<float>(Tcw, 48); auto oO = s.out<float>(Ow, 12);
    // a call that does not converge leaves the pose, and one with too few correspondences everything but the header, as it was: the caller's arrays go
    // up first so that they come back unchanged
    for (int i = of.i; i < s.n; ++i) s.pc[i].src = s.pc[i].dst;
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_sim3_solve_device(c, 1, n1, M, pt, p1, mt, t1, 0, t2, cam1, cam2, max_err1, max_err2, fix_scale, min_inliers, 0, nullptr, tb, max_iters, dr, 0,
                                         rand_max, (unsigned char*)ws, oh, of, oi, oT, oO);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

int xfh_sim3_merge_matches_host(int J, int n1, int n2, int M, const int* match12, const int* point2, void* workspace, int* matched, int* matched_kf,
                                int* num_matches) {
    if (!s3_merge_dims_ok(J, n1, n2, M) || !match12 || !point2 || !workspace || !matched || !matched_kf || !num_matches) return XFH_ERR_INVALID_ARG;
    if (misaligned(3, match12, point2, matched, matched_kf, num_matches) || misaligned(15, workspace)) return XFH_ERR_INVALID_ARG;
    s3_merge_host(J, n1, n2, M, match12, point2, (int*)workspace, matched, matched_kf, num_matches);
    return XFH_OK;
}

int xfh_sim3_merge_matches_device(xfh_ctx* c, int J, int n1, int n2, int M, const int* d_match12, const int* d_point2, void* d_workspace, int* d_matched,
                                  int* d_matched_kf, int* d_num_matches) {
    if (!c || !s3_merge_dims_ok(J, n1, n2, M) || !d_match12 || !d_point2 || !d_workspace || !d_matched || !d_matched_kf || !d_num_matches) return XFH_ERR_INVALID_ARG;
    if (misaligned(3, d_match12, d_point2, d_matched, d_matched_kf, d_num_matches) || misaligned(15, d_workspace)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const S3MergeArgs a{J, n1, n2, M, d_match12, d_point2, (int*)d_workspace, d_matched, d_matched_kf, d_num_matches};
    HIPCK(c, launch_sim3_merge(c, a));
    return XFH_OK;
}

int xfh_sim3_merge_matches(xfh_ctx* c, int J, int n1, int n2, int M, const int* match12, const int* point2, int* matched, int* matched_kf, int* num_matches) {
    if (!c || !s3_merge_dims_ok(J, n1, n2, M) || !match12 || !point2 || !matched || !matched_kf || !num_matches) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto m = s.in<int>(match12, (size_t)J * n1 * 4); auto p2 = s.in<int>(point2, (size_t)J * n2 * 4); auto ws = s.tmp<unsigned char>(geo_al16((size_t)M * 4));
    auto o0 = s.out<int>(matched, (size_t)n1 * 4); auto o1 = s.out<int>(matched_kf, (size_t)n1 * 4); auto o2 = s.out<int>(num_matches, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_sim3_merge_matches_device(c, J, n1, n2, M, m, p2, (unsigned char*)ws, o0, o1, o2);
    if (rc != XFH_OK) return rc;
    return s.download();
}

}  // extern "C"

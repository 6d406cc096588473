// capi_twoview.cpp -- the entry points of include/xfeat_hip.h behind TwoViewReconstruction::Reconstruct of monocular initialisation
// (xfh_two_view*): the pieces of the rule on the host (twoview_math.h, the kernels' own lines), the whole rule on one host thread, the device
// form and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "twoview_math.h"
#include <math.h>
#include <vector>

static bool tv_dims_ok(int B, int n1, int n2, int iters) {
    return B >= 1 && B <= 65535 && n1 >= 1 && n1 <= XFH_GRID_MAX_N && n2 >= 1 && n2 <= XFH_GRID_MAX_N && iters >= 1 && iters <= TV_MAX_ITERS;
}
static bool tv_scalars_ok(const xfh_camera* cam, float sigma, int rand_max, double min_parallax_cos, int min_triangulated) {
    return cam && isfinite(sigma) && sigma > 0.0f && rand_max >= 1 && isfinite(min_parallax_cos) && min_triangulated >= 0;
}
static bool tv_stride_ok(int B, int iters, size_t stride) { return stride == 0 || stride >= (size_t)iters * 8 || B == 1; }
static bool tv_model_ok(int model) { return model == XFH_TWO_VIEW_MODEL_H || model == XFH_TWO_VIEW_MODEL_F; }

static TvArgs tv_args(int B, int n1, int n2, const float* xy1, const float* xy2, const int* matches12, const xfh_camera* cam, float sigma, int iters,
                      const int* draws, size_t stride, int rand_max, double min_parallax_cos, int min_triangulated, void* ws, int* header, float* floats,
                      uint8_t* inl_h, uint8_t* inl_f, uint8_t* tri, float* p3d, int* matches_out) {
    TvArgs a = {};
    a.B = B; a.n1 = n1; a.n2 = n2; a.iters = iters; a.rand_max = rand_max; a.min_tri = min_triangulated; a.draws_stride = stride;
    a.cam = GeoCam{cam->fx, cam->fy, cam->cx, cam->cy}; a.sigma = sigma; a.min_parallax_cos = min_parallax_cos;
    a.xy1 = xy1; a.xy2 = xy2; a.match12 = matches12; a.draws = draws; a.ws = (unsigned char*)ws;
    a.header = header; a.fout = floats; a.inl_h = inl_h; a.inl_f = inl_f; a.tri = tri; a.p3d = p3d; a.matches_out = matches_out;
    return a;
}

extern "C" {

size_t xfh_two_view_workspace_bytes(int n1, int n2, int iters, int B) {
    if (!tv_dims_ok(B, n1, n2, iters)) return 0;
    return tv_layout(n1, iters).per_problem * (size_t)B;
}

int xfh_two_view_set(const int* draws8, int rand_max, int N, int* set8) {
    if (!draws8 || !set8 || rand_max < 1 || N < 8) return XFH_ERR_INVALID_ARG;
    geo_set<TV_MIN_SET>(draws8, rand_max, N, set8);
    return XFH_OK;
}

int xfh_two_view_fit(int model, const float* xy1n, const float* xy2n, float* M) {
    if (!tv_model_ok(model) || !xy1n || !xy2n || !M) return XFH_ERR_INVALID_ARG;
    double u[144], v[81];
    const GeoMat U{u, 1}, V{v, 1};
    if (model == TV_MODEL_H) tv_fit_h(xy1n, xy2n, U, V, M); else tv_fit_f(xy1n, xy2n, U, V, M);
    return XFH_OK;
}

int xfh_two_view_score(int model, const float* M, float sigma, const float* xy1, const float* xy2, float* chi2, int* inlier, float* term) {
    if (!tv_model_ok(model) || !M || !xy1 || !xy2 || !chi2 || !inlier || !term || !isfinite(sigma) || !(sigma > 0.0f)) return XFH_ERR_INVALID_ARG;
    *term = tv_score(model, M, tv_inv_sigma2(sigma), xy1[0], xy1[1], xy2[0], xy2[1], chi2, inlier);
    return XFH_OK;
}

int xfh_two_view_check_rt(const xfh_camera* cam, const float* T21, float sigma, const float* xy1, const float* xy2, int* verdict, float* cos_parallax,
                          float* p3d) {
    if (!cam || !T21 || !xy1 || !xy2 || !verdict || !cos_parallax || !p3d || !isfinite(sigma) || !(sigma > 0.0f)) return XFH_ERR_INVALID_ARG;
    *verdict = tv_check_rt_pair(GeoCam{cam->fx, cam->fy, cam->cx, cam->cy}, T21, tv_th2(sigma), xy1[0], xy1[1], xy2[0], xy2[1], cos_parallax, p3d);
    return XFH_OK;
}

int xfh_two_view_host(int B, int n1, int n2, const float* xy1, const float* xy2, const int* matches12, const xfh_camera* cam, float sigma, int iters,
                      const int* draws, size_t draws_problem_stride, int rand_max, double min_parallax_cos, int min_triangulated, void* workspace,
                      int* header, float* floats, uint8_t* inlier_h, uint8_t* inlier_f, uint8_t* triangulated, float* p3d, int* matches_out) {
    if (!tv_dims_ok(B, n1, n2, iters) || !tv_scalars_ok(cam, sigma, rand_max, min_parallax_cos, min_triangulated) || !tv_stride_ok(B, iters, draws_problem_stride))
        return XFH_ERR_INVALID_ARG;
    if (!xy1 || !xy2 || !matches12 || !draws || !workspace || !header || !floats || !inlier_h || !inlier_f || !triangulated || !p3d || !matches_out)
        return XFH_ERR_INVALID_ARG;
    if (misaligned(3, xy1, xy2, matches12, draws, header, floats, p3d, matches_out) || misaligned(15, workspace)) return XFH_ERR_INVALID_ARG;
    const TvArgs a = tv_args(B, n1, n2, xy1, xy2, matches12, cam, sigma, iters, draws, draws_problem_stride, rand_max, min_parallax_cos, min_triangulated,
                             workspace, header, floats, inlier_h, inlier_f, triangulated, p3d, matches_out);
    std::vector<float> scratch((size_t)(n1 > n2 ? n1 : n2));
    for (int b = 0; b < B; ++b) tv_host_problem(a, b, scratch.data());
    return XFH_OK;
}

int xfh_two_view_device(xfh_ctx* c, int B, int n1, int n2, const float* d_xy1, const float* d_xy2, const int* d_matches12, const xfh_camera* cam,
                        float sigma, int iters, const int* d_draws, size_t draws_problem_stride, int rand_max, double min_parallax_cos,
                        int min_triangulated, void* d_workspace, int* d_header, float* d_floats, uint8_t* d_inlier_h, uint8_t* d_inlier_f,
                        uint8_t* d_triangulated, float* d_p3d, int* d_matches_out) {
    if (!c || !tv_dims_ok(B, n1, n2, iters) || !tv_scalars_ok(cam, sigma, rand_max, min_parallax_cos, min_triangulated) ||
        !tv_stride_ok(B, iters, draws_problem_stride)) return XFH_ERR_INVALID_ARG;
    if (!d_xy1 || !d_xy2 || !d_matches12 || !d_draws || !d_workspace || !d_header || !d_floats || !d_inlier_h || !d_inlier_f || !d_triangulated || !d_p3d ||
        !d_matches_out) return XFH_ERR_INVALID_ARG;
    if (misaligned(3, d_xy1, d_xy2, d_matches12, d_draws, d_header, d_floats, d_p3d, d_matches_out) || misaligned(15, d_workspace)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const TvArgs a = tv_args(B, n1, n2, d_xy1, d_xy2, d_matches12, cam, sigma, iters, d_draws, draws_problem_stride, rand_max, min_parallax_cos,
                             min_triangulated, d_workspace, d_header, d_floats, d_inlier_h, d_inlier_f, d_triangulated, d_p3d, d_matches_out);
    HIPCK(c, launch_two_view(c, a));
    return XFH_OK;
}

int xfh_two_view(xfh_ctx* c, int n1, int n2, const float* xy1, const float* xy2, const int* matches12, const xfh_camera* cam, float sigma, int iters,
                 const int* draws, int rand_max, double min_parallax_cos, int min_triangulated, int* header, float* floats, uint8_t* inlier_h,
                 uint8_t* inlier_f, uint8_t* triangulated, float* p3d, int* matches_out) {
    if (!c || !tv_dims_ok(1, n1, n2, iters) || !tv_scalars_ok(cam, sigma, rand_max, min_parallax_cos, min_triangulated)) return XFH_ERR_INVALID_ARG;
    if (!xy1 || !xy2 || !matches12 || !draws || !header || !floats || !inlier_h || !inlier_f || !triangulated || !p3d || !matches_out) return XFH_ERR_INVALID_ARG;
    const size_t N1 = (size_t)n1, N2 = (size_t)n2;
    HostStage s{c};
    auto x1 = s.in<float>(xy1, N1 * 8); auto x2 = s.in<float>(xy2, N2 * 8); auto m = s.in<int>(matches12, N1 * 4); auto dr = s.in<int>(draws, (size_t)iters * 32);
    auto ws = s.tmp<unsigned char>(xfh_two_view_workspace_bytes(n1, n2, iters, 1));
    auto oh = s.out<int>(header, TV_HEADER_INTS * 4); auto of = s.out<float>(floats, TV_FLOATS * 4); auto o1 = s.out<uint8_t>(inlier_h, N1);
    auto o2 = s.out<uint8_t>(inlier_f, N1); auto o3 = s.out<uint8_t>(triangulated, N1); auto op = s.out<float>(p3d, N1 * 12); auto om = s.out<int>(matches_out, N1 * 4);
    // with fewer than eight matches only the header is written: the caller's other arrays go up first so that they come back as they were
    for (int i = of.i; i < s.n; ++i) s.pc[i].src = s.pc[i].dst;            // every output behind the header
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_two_view_device(c, 1, n1, n2, x1, x2, m, cam, sigma, iters, dr, 0, rand_max, min_parallax_cos, min_triangulated, (unsigned char*)ws, oh, of,
                                       o1, o2, o3, op, om);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"

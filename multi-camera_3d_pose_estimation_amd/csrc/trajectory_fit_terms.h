// The trajectory fit's data term, under the kernels of trajectory_fit_kernels.h: the observation
// arguments, one frame's terms at a state, and the argument checks of the entry points.
#pragma once
#include "trajectory_fit_solver.h"
#include "refine_common.h"

namespace {

struct FitObs {
    ReprojObs obs;          // kpts [T][P][3][V], mask [T][P], gauss [T][V][P][6]; stride P: e = t·P + p
    ViewList vl;
    const double* cams;
    int T, P, n_cams;
};

// One frame's terms at X: the used views' Σ rho, Σ s², their count, whether X is in front of all of
// them; with JAC the data terms H̃ and g̃.
struct FitFrame {
    double rho, s2, H[6], g[3];
    int nviews;
    bool front;
};

template <bool JAC>
__device__ __forceinline__ void fit_frame(const FitObs& o, const double (*scam)[MVP_CAM_DOUBLES], int t, int p,
                                          const double (&X)[3], FitFrame& f) {
#pragma clang fp contract(fast)
    const int64_t e = (int64_t)t * o.P + p;
    const unsigned allowed = reproj_allowed(o.obs, e);
    f.rho = 0.0, f.s2 = 0.0, f.nviews = 0, f.front = true;
#pragma unroll
    for (int k = 0; k < 6; k++) f.H[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) f.g[k] = 0.0;
#pragma unroll 1
    for (int j = 0; j < o.vl.nv; j++) {
        const int col = o.vl.col(j);
        double zx, zy, wxx, wxy, wyy;
        const bool u = reproj_observe(o.obs, e, t, p, col, (allowed >> j) & 1u, zx, zy, wxx, wxy, wyy);
        const RefineCam c = refine_cam(&scam[col][0]);
        double rho = 0.0, s2 = 0.0, g[3] = {0, 0, 0}, H[6] = {0, 0, 0, 0, 0, 0};
        const bool infront = refine_view_terms_huber<JAC>(c, X, zx, zy, wxx, wxy, wyy, o.obs.hub, rho, s2, g, H);
        f.front = f.front && (infront || !u);
        f.nviews += u ? 1 : 0;
        f.rho += u ? rho : 0.0;
        f.s2 += u ? s2 : 0.0;
        if (JAC) {
#pragma unroll
            for (int k = 0; k < 3; k++) f.g[k] += u ? g[k] : 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) f.H[k] += u ? H[k] : 0.0;
        }
    }
}

// The checks the device calls share; returns the observation arguments.
inline FitObs fit_parse(const char* fn, const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                        const int* cam_idx, int nv, const uint8_t* mask, int weights, const double* gauss,
                        float min_conf, float cov_floor, double huber_delta) {
    MVP_REQUIRE(T >= 1, "%s: T=%d < 1", fn, T);
    MVP_REQUIRE(P >= 1, "%s: P=%d < 1", fn, P);
    MVP_REQUIRE((int64_t)T * P < (1LL << 31), "%s: T·P=%lld must be < 2^31", fn, (long long)T * P);
    const CamIdx ci = tri_parse_args(fn, (int64_t)T * P, V, n_cams, cam_idx, nv);
    FitObs o{};
    o.obs = reproj_parse_obs(fn, kpts, (int64_t)T * P, V, mask, weights, gauss, P, min_conf, cov_floor, huber_delta);
    o.vl = view_list(ci, nv);
    o.cams = cams, o.T = T, o.P = P, o.n_cams = n_cams;
    return o;
}

}  // namespace

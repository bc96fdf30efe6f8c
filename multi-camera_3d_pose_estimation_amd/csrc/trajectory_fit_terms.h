// The trajectory fit's data term, under the kernels of trajectory_fit_kernels.h: the observation
// arguments, one frame's terms at a state, and the argument checks of the entry points.
#pragma once
#include "trajectory_fit_solver.h"
#include "refine_common.h"

namespace {

struct FitObs {
    const float* kpts;      // [T][P][3][V]
    const uint8_t* mask;    // [T][P] or null
    const double* gauss;    // [T][V][P][6] or null
    const double* cams;
    int T, P, V, n_cams, nv, weights;
    unsigned cols;          // the listed cameras as nibbles
    float min_conf, cov_floor;
    double hub;
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
    const float* __restrict__ kp = o.kpts + e * 3 * o.V;
    const unsigned allowed = o.mask ? (unsigned)o.mask[e] : 0xFFu;
    f.rho = 0.0, f.s2 = 0.0, f.nviews = 0, f.front = true;
#pragma unroll
    for (int k = 0; k < 6; k++) f.H[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) f.g[k] = 0.0;
#pragma unroll 1
    for (int j = 0; j < o.nv; j++) {
        const int col = (o.cols >> (4 * j)) & 15u;
        double zx, zy, wxx, wxy, wyy;
        const bool u = refine_observation(kp, o.V, col, (allowed >> j) & 1u, o.weights, o.gauss, t, p, o.P, o.min_conf,
                                          o.cov_floor, zx, zy, wxx, wxy, wyy);
        const RefineCam c = refine_cam(&scam[col][0]);
        double rho = 0.0, s2 = 0.0, g[3] = {0, 0, 0}, H[6] = {0, 0, 0, 0, 0, 0};
        const bool infront = refine_view_terms_huber<JAC>(c, X, zx, zy, wxx, wxy, wyy, o.hub, rho, s2, g, H);
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

// The checks the two device calls share; returns the observation arguments.
inline FitObs fit_parse(const char* fn, const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                        const int* cam_idx, int nv, const uint8_t* mask, int weights, const double* gauss,
                        float min_conf, float cov_floor, double huber_delta) {
    MVP_REQUIRE(T >= 1, "%s: T=%d < 1", fn, T);
    MVP_REQUIRE(P >= 1, "%s: P=%d < 1", fn, P);
    MVP_REQUIRE((int64_t)T * P < (1LL << 31), "%s: T·P=%lld must be < 2^31", fn, (long long)T * P);
    const CamIdx ci = tri_parse_args(fn, (int64_t)T * P, V, n_cams, cam_idx, nv);
    MVP_REQUIRE(weights >= MVP_REFINE_W_UNIT && weights <= MVP_REFINE_W_GAUSS, "%s: weights=%d (0..2)", fn, weights);
    if (weights == MVP_REFINE_W_GAUSS) MVP_REQUIRE(gauss != nullptr, "%s: MVP_REFINE_W_GAUSS needs gauss_dev", fn);
    MVP_REQUIRE(!std::isnan(min_conf), "%s: min_conf is NaN", fn);
    MVP_REQUIRE(cov_floor >= 0.f, "%s: cov_floor=%g (not NaN, >= 0)", fn, (double)cov_floor);
    MVP_REQUIRE(!std::isnan(huber_delta), "%s: huber_delta is NaN", fn);
    FitObs o{};
    o.kpts = kpts, o.mask = mask, o.gauss = gauss, o.cams = cams;
    o.T = T, o.P = P, o.V = V, o.n_cams = n_cams, o.nv = nv, o.weights = weights;
    for (int j = 0; j < nv; j++) o.cols |= (unsigned)ci.v[j] << (4 * j);
    o.min_conf = min_conf, o.cov_floor = cov_floor;
    o.hub = huber_delta > 0 ? huber_delta : 0.0;
    return o;
}

}  // namespace

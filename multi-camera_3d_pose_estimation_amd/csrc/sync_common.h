// The two staging launches shared by the epipolar kernels (sync.hip: mvp_epipolar_lag_cost;
// associate.hip: mvp_associate_views): the fundamental matrix of every pair of listed views and
// the float32 undistorted pixel of every keypoint, NaN where the keypoint is not usable.  Both are
// stated in include/mvpose.h ("Epipolar lag-cost scan").
#pragma once
#pragma clang fp contract(off)

#include "tri_common.h"

namespace {

constexpr int kSyMaxPairs = kMaxCams * (kMaxCams - 1) / 2;

struct SyncPairs {
    unsigned char a[kSyMaxPairs], b[kSyMaxPairs];   // positions in cam_idx
};

// (a, b), a < b positions in cam_idx, in lexicographic order; returns their number.
inline int sync_list_pairs(int nv, SyncPairs& pr) {
    int np = 0;
    for (int a = 0; a < nv; a++)
        for (int b = a + 1; b < nv; b++) {
            pr.a[np] = (unsigned char)a;
            pr.b[np] = (unsigned char)b;
            np++;
        }
    return np;
}

inline int64_t sy_align256(int64_t b) { return (b + 255) / 256 * 256; }

// inverse of a 3x3 matrix by its adjugate (row-major)
__device__ __forceinline__ void inv3(const double* m, double (&o)[9]) {
    const double c0 = m[4] * m[8] - m[5] * m[7];
    const double c1 = m[5] * m[6] - m[3] * m[8];
    const double c2 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    const double id = 1.0 / det;
    o[0] = c0 * id;
    o[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c1 * id;
    o[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c2 * id;
    o[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// F_ab = K_b⁻ᵀ [t]ₓ R K_a⁻¹, R = R_b R_aᵀ, t = T_b − R T_a: x_bᵀ F x_a = 0 for matched pixels.
__global__ void sync_fundamental_kernel(const double* __restrict__ cams, CamIdx ci, SyncPairs pr, int n_pairs,
                                        double* __restrict__ fmat) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const double* ca = cams + (int64_t)ci.v[pr.a[p]] * MVP_CAM_DOUBLES;
    const double* cb = cams + (int64_t)ci.v[pr.b[p]] * MVP_CAM_DOUBLES;
    const double *Ra = ca + 14, *Ta = ca + 23, *Rb = cb + 14, *Tb = cb + 23;
    double R[9], t[3], E[9], Kai[9], Kbi[9], M[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = Rb[3 * i] * Ra[3 * j] + Rb[3 * i + 1] * Ra[3 * j + 1] + Rb[3 * i + 2] * Ra[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = Tb[i] - (R[3 * i] * Ta[0] + R[3 * i + 1] * Ta[1] + R[3 * i + 2] * Ta[2]);
    // E = [t]ₓ R
#pragma unroll
    for (int j = 0; j < 3; j++) {
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
    inv3(ca, Kai);
    inv3(cb, Kbi);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[3 * i + j] = E[3 * i] * Kai[j] + E[3 * i + 1] * Kai[3 + j] + E[3 * i + 2] * Kai[6 + j];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) fmat[9 * p + 3 * i + j] = Kbi[i] * M[j] + Kbi[3 + i] * M[3 + j] + Kbi[6 + i] * M[6 + j];
}

// und[i][e] = the f32 undistorted pixel of view i's keypoint e (a (t, j) or a (t, slot, j) index:
// the keypoint's three rows start at kpts + e·3·V), NaN when not usable.
__global__ __launch_bounds__(kBlock) void sync_undistort_kernel(const float* __restrict__ kpts, int64_t n, int V,
                                                                const double* __restrict__ cams, int n_cams,
                                                                CamIdx ci, float min_conf, float2* __restrict__ und) {
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    load_cams(scam, sfast, cams, n_cams);  // ends in the block's barrier
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int col = ci.v[blockIdx.y];
    const float* __restrict__ kp = kpts + e * 3 * V;
    const float x = kp[col], y = kp[V + col], c = kp[2 * V + col];
    float ux, uy;
    undistort_point(x, y, scam[col], ux, uy);
    const bool ok = view_usable(x, y, c, min_conf);
    const float qnan = __builtin_nanf("");
    und[(int64_t)blockIdx.y * n + e] = make_float2(ok ? ux : qnan, ok ? uy : qnan);
}

}  // namespace

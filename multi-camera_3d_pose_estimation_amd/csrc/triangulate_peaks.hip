// mvp_triangulate_peaks: the robust N-view triangulation over several 2D candidates per view
// (mvp_heatmap_peaks' modes), choosing one candidate per inlier view (numerics contract and shared
// device code in tri_common.h; algorithm in mvpose.h; map of the triangulation files in
// triangulate.hip).
#pragma clang fp contract(off)

#include "tri_common.h"

namespace {

// One lane per point, as the robust kernel, and the same solver code: step A and the final solve
// of step B are ONE copy of the all-views solver inside a two-trip loop over a view mask, the
// rows of the views outside the mask exact zeros.
//   * Undistorted candidates are parked in LDS, [view][slot][lane] (bank-conflict free): step B
//     indexes views and slots at run time.  8 views x 4 slots x 8 B = 256 B per lane, so the block
//     is 128 lanes (32 KB at NV = 8); scores are read again from global memory where needed.
//   * Step A undistorts slot 0 of every view, branch-free like the robust kernel, and goes on to
//     the later slots only for the views whose slot 0 is no valid candidate: on clean points the
//     extra slots cost their bytes and nothing else.
//   * Step B is entered under a wave ballot.  It undistorts the remaining candidates, then scores
//     every (a, b, ma, mb) hypothesis (one-sided Jacobi on the 4x4 two-view DLT: only selects, no
//     bit contract) against each valid view's nearest valid candidate.
//   * out_kpts is written by the whole block in one coalesced pass over the block's points, the
//     points' masks and selections handed over through LDS.
// sel packs the chosen slot of view j in bits 2j, 2j+1; cval holds bit 4j + m for a valid
// candidate (view j, slot m).
constexpr int kPeakBlock = 128;
static_assert(MVP_MAX_PEAKS == 4, "sel packs a slot in 2 bits, cval a view in 4");

template <int NV>
__global__ __launch_bounds__(kPeakBlock) __attribute__((amdgpu_waves_per_eu(NV == 8 ? 2 : 1))) void triangulate_peaks_kernel(
    const float* __restrict__ peaks, int64_t n, int M, int V, const double* __restrict__ cams, int n_cams, CamIdx ci,
    float inlier_px, float min_conf, float* __restrict__ out, uint8_t* __restrict__ out_mask,
    int8_t* __restrict__ out_sel, float* __restrict__ out_err, float* __restrict__ out_kpts) {
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    __shared__ int scol[kMaxCams];
    __shared__ float s_ux[NV][MVP_MAX_PEAKS][kPeakBlock], s_uy[NV][MVP_MAX_PEAKS][kPeakBlock];
    __shared__ int s_pos[64];                    // column -> view position, -1 for a column that is not listed
    __shared__ unsigned s_mask[kPeakBlock], s_sel[kPeakBlock];  // the points' results, for the out_kpts pass
#pragma unroll
    for (int j = 0; j < NV; j++)
        if ((int)threadIdx.x == j) scol[j] = ci.v[j];
    if (threadIdx.x == 0) {
        for (int c = 0; c < V; c++) s_pos[c] = -1;
#pragma unroll
        for (int j = 0; j < NV; j++) s_pos[ci.v[j]] = j;  // a column listed twice: its last position
    }
    load_cams(scam, sfast, cams, n_cams);  // ends in the block's barrier
    // the lanes past the last point solve it once more and write nothing: every lane reaches the
    // block's barrier before the out_kpts pass
    const int64_t p0 = (int64_t)blockIdx.x * kPeakBlock + threadIdx.x;
    const bool live = p0 < n;
    const int64_t p = live ? p0 : n - 1;
    const int tid = threadIdx.x;
    const float* __restrict__ kp = peaks + p * M * 3 * V;
    const double inl = (double)inlier_px;
    // candidate (column col, slot m): undistorted into LDS row [j][m]; returns its validity
    auto park = [&](int j, int col, int m) {
        const float* __restrict__ c = kp + (size_t)m * 3 * V + col;
        const float x = c[0], y = c[V], s = c[2 * V];
        float ux, uy;
        undistort_point_fast(x, y, scam[col], sfast[col], ux, uy);
        s_ux[j][m][tid] = ux;
        s_uy[j][m][tid] = uy;
        return view_usable(x, y, s, min_conf) && isfinite(ux) && isfinite(uy);
    };
    unsigned valid = 0, sel = 0;
#pragma unroll
    for (int j = 0; j < NV; j++) valid |= (park(j, ci.v[j], 0) ? 1u : 0u) << j;
    const unsigned ok0 = valid;
    if (M > 1) {
#pragma unroll 1
        for (int j = 0; j < NV; j++) {
            if ((valid >> j) & 1u) continue;
#pragma unroll 1
            for (int m = 1; m < M; m++)
                if (park(j, scol[j], m)) {
                    valid |= 1u << j;
                    sel |= (unsigned)m << (2 * j);
                    break;
                }
        }
    }
    const float qnan = __builtin_nanf("");
    unsigned mask = valid;                  // the views of the next solve
    unsigned cval = 0;                      // every valid candidate: known from step B on
    bool active = __popc(valid) >= 2;       // this lane takes part in the next solve
    bool failed = !active;                  // NaN point, empty mask
    float xyz[3] = {qnan, qnan, qnan};
    float err[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) err[j] = qnan;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        bool all_in = true;
        if (active) {
            double nv[4];
            {
                double A[2 * NV][4];
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    if ((mask >> j) & 1u) {
                        const int m = (sel >> (2 * j)) & 3u;
                        add_view_rows(A, 2 * j, s_ux[j][m][tid], s_uy[j][m][tid], scam[ci.v[j]] + 26);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) A[2 * j][k] = A[2 * j + 1][k] = 0.0;
                    }
                }
                dlt_null_vector<false, 2 * NV>(A, nv);
            }
            dehomogenize_f32(nv, xyz);
            const double X[4] = {(double)xyz[0], (double)xyz[1], (double)xyz[2], 1.0};
#pragma unroll
            for (int j = 0; j < NV; j++)
                if ((valid >> j) & 1u) {
                    const double* __restrict__ P = scam[ci.v[j]] + 26;
                    double e;
                    if ((mask >> j) & 1u) {
                        const int m = (sel >> (2 * j)) & 3u;
                        e = reprojection_error(P, X, s_ux[j][m][tid], s_uy[j][m][tid]);
                    } else {  // pass 1 only (pass 0 solves over every valid view): the nearest valid candidate
                        e = (double)INFINITY;
#pragma unroll 1
                        for (int m = 0; m < M; m++)
                            if ((cval >> (4 * j + m)) & 1u) {
                                const double em = reprojection_error(P, X, s_ux[j][m][tid], s_uy[j][m][tid]);
                                if (em < e) e = em;
                            }
                    }
                    err[j] = (float)e;
                    all_in = all_in && (e <= inl);
                }
        }
        if (pass == 1) break;
        const bool need_b = active && !all_in;
        if (__ballot(need_b) == 0) break;  // every point of the wave accepted in step A (or has < 2 views)
        active = need_b;
        if (need_b) {
            cval = 0;
#pragma unroll 1
            for (int j = 0; j < NV; j++) {
                if ((valid >> j) & 1u) cval |= ((ok0 >> j) & 1u) << (4 * j);
#pragma unroll 1
                for (int m = 1; m < M; m++)
                    if (((valid >> j) & 1u) && park(j, scol[j], m)) cval |= 1u << (4 * j + m);
            }
            int best_cnt = -1;
            float best_sum = 0.f;
            unsigned best_mask = 0, best_sel = 0;
#pragma unroll 1
            for (int a = 0; a < NV - 1; a++) {
#pragma unroll 1
                for (int b = a + 1; b < NV; b++) {
                    if (!(((valid >> a) & 1u) && ((valid >> b) & 1u))) continue;
                    const double* __restrict__ Pa = scam[scol[a]] + 26;
                    const double* __restrict__ Pb = scam[scol[b]] + 26;
#pragma unroll 1
                    for (int mab = 0; mab < M * M; mab++) {
                        const int ma = mab / M, mb = mab - ma * M;
                        if (!(((cval >> (4 * a + ma)) & 1u) && ((cval >> (4 * b + mb)) & 1u))) continue;
                        const double xa = s_ux[a][ma][tid], ya = s_uy[a][ma][tid];
                        const double xb = s_ux[b][mb][tid], yb = s_uy[b][mb][tid];
                        double At[4][4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            At[k][0] = xa * Pa[8 + k] - Pa[0 + k];
                            At[k][1] = ya * Pa[8 + k] - Pa[4 + k];
                            At[k][2] = xb * Pb[8 + k] - Pb[0 + k];
                            At[k][3] = yb * Pb[8 + k] - Pb[4 + k];
                        }
                        double X[4];
                        jacobi_null_vector<4>(At, X);
                        int cnt = 0;
                        float sum = 0.f;  // f32, ascending view position
                        unsigned hm = 0, hs = 0;
#pragma unroll
                        for (int j = 0; j < NV; j++)
                            if ((valid >> j) & 1u) {
                                const double* __restrict__ P = scam[ci.v[j]] + 26;
                                double e = (double)INFINITY;
                                int ms = -1;
#pragma unroll 1
                                for (int m = 0; m < M; m++)
                                    if ((cval >> (4 * j + m)) & 1u) {
                                        const double em = reprojection_error(P, X, s_ux[j][m][tid], s_uy[j][m][tid]);
                                        if (ms < 0 || em < e) {  // ties go to the lower slot
                                            e = em;
                                            ms = m;
                                        }
                                    }
                                if (e <= inl) {
                                    cnt++;
                                    sum = __fadd_rn(sum, kp[((size_t)ms * 3 + 2) * V + ci.v[j]]);
                                    hm |= 1u << j;
                                    hs |= (unsigned)ms << (2 * j);
                                }
                            }
                        if (cnt > best_cnt || (cnt == best_cnt && sum > best_sum)) {
                            best_cnt = cnt;
                            best_sum = sum;
                            best_mask = hm;
                            best_sel = hs;
                        }
                    }
                }
            }
            if (best_cnt < 2) {
                failed = true;
                active = false;
            } else {
                mask = best_mask;
                sel = best_sel;
            }
        }
    }
    if (failed) {
        mask = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) xyz[k] = qnan;
#pragma unroll
        for (int j = 0; j < NV; j++) err[j] = qnan;
    }
    if (live) {
        out[3 * p + 0] = xyz[0];
        out[3 * p + 1] = xyz[1];
        out[3 * p + 2] = xyz[2];
        out_mask[p] = (uint8_t)mask;
#pragma unroll
        for (int j = 0; j < NV; j++)
            out_sel[p * NV + j] = ((mask >> j) & 1u) ? (int8_t)((sel >> (2 * j)) & 3u) : (int8_t)-1;
        if (out_err) {
#pragma unroll
            for (int j = 0; j < NV; j++) out_err[p * NV + j] = err[j];
        }
    }
    if (!out_kpts) return;  // uniform
    // out_kpts of the block's points is one contiguous run of 3·V floats per point: written by the
    // whole block, consecutive lanes consecutive floats, each float from slot 0 or, in a masked
    // view's column, from the slot its point selected (measured against one lane per point writing
    // its 3·V floats: DESIGN §4.19)
    s_mask[tid] = mask;
    s_sel[tid] = sel;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * kPeakBlock;
    const int w3 = 3 * V;
    const int total = (int)min((int64_t)kPeakBlock, n - first) * w3;  // <= 128 · 192
    const float* __restrict__ src = peaks + first * M * w3;
    float* __restrict__ dst = out_kpts + first * w3;
    for (int i = tid; i < total; i += kPeakBlock) {
        const int q = i / w3, r = i - q * w3, col = r % V;
        const int j = s_pos[col];
        const int m = (j >= 0 && ((s_mask[q] >> j) & 1u)) ? (int)((s_sel[q] >> (2 * j)) & 3u) : 0;
        dst[i] = src[((size_t)q * M + m) * w3 + r];
    }
}

}  // namespace

extern "C" int mvp_triangulate_peaks(const float* peaks, int64_t n_points, int M, int V, const double* cams,
                                     int n_cams, const int* cam_idx, int n_cam_idx, float inlier_px, float min_conf,
                                     float* out_xyz, uint8_t* out_mask, int8_t* out_sel, float* out_err,
                                     float* out_kpts, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_triangulate_peaks";
    const CamIdx ci = tri_parse_args(fn, n_points, V, n_cams, cam_idx, n_cam_idx);
    MVP_REQUIRE(M >= 1 && M <= MVP_MAX_PEAKS, "mvp_triangulate_peaks: M=%d (1..%d)", M, MVP_MAX_PEAKS);
    MVP_REQUIRE(std::isfinite(inlier_px) && inlier_px > 0.f, "mvp_triangulate_peaks: inlier_px=%g (finite, > 0)",
                (double)inlier_px);
    MVP_REQUIRE(!std::isnan(min_conf), "mvp_triangulate_peaks: min_conf is NaN");
    if (n_points == 0) return MVP_OK;
    MVP_REQUIRE(peaks && cams && out_xyz && out_mask && out_sel, "mvp_triangulate_peaks: null device pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t blocks = (n_points + kPeakBlock - 1) / kPeakBlock;
    MVP_REQUIRE(blocks < (1LL << 31), "mvp_triangulate_peaks: too many points");
    const dim3 grid((unsigned)blocks), block(kPeakBlock);
    tri_dispatch_views(n_cam_idx, [&](auto nv) {
        hipLaunchKernelGGL((triangulate_peaks_kernel<decltype(nv)::value>), grid, block, 0, s, peaks, n_points, M, V,
                           cams, n_cams, ci, inlier_px, min_conf, out_xyz, out_mask, out_sel, out_err, out_kpts);
    });
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

// Trajectories fitted to the 2D keypoints (mvp_trajectory_fit_plan / _system / mvp_trajectory_fit;
// the problem is stated in include/mvpose.h; no reference counterpart) for gfx950.
//
// Per chain p, Levenberg-Marquardt on
//   f(X) = Σ_t Σ_used rho(reprojection of X_t in view i) + ½ λ Σ_{t>=2} |X_t − 2 X_{t−1} + X_{t−2}|².
// A Gauss-Newton step of it is the block-pentadiagonal system the smoother solves, with the frames'
// 3x3 information blocks H̃_t where the smoother has W_t: frames seen by one view enter with their
// rank-2 block, frames seen by none with nothing, and the prior carries them.  Stream-ordered
// launches, arithmetic in fp64, FMA contraction on (no bit contract), no floating-point atomics.
// The kernels are trajectory_fit_kernels.h's with no coupling between chains (NoCoupling) and
// smooth_solver.h's over trajectory_fit_solver.h's frame source:
//
//   fit_prepare_kernel<2>   one lane per (t, p): the f64 copy of the seed, the number of used views,
//              and the two numbers a chain's validity is summed from (frames with >= 2 used views;
//              frames whose seed is not finite or lies behind a used view).
//   fit_terms_kernel<JAC, NoCoupling>   one lane per (t, p), lanes along p, the camera records in
//              LDS: the used views' rho, and with JAC the frame's H̃ (6) and the right-hand side
//              −(g̃ + λ·(D₂ᵀD₂ X)_t) (3), read from the fp64 state at t±1, t±2.  Writes the frame's
//              two cost terms (Σ rho, or +inf behind a camera; the prior's row t).  The used set
//              depends on the keypoints alone (refine_common.h's rule), so it is re-derived, not
//              stored.
//   fit_sum_kernel<2>   per chain, the frames' two numbers in tiles of 256 frames: each of a
//              workgroup's 4 rows of lanes adds its frames in ascending order, the rows are added
//              in order.
//   fit_decide_kernel   (trajectory_fit_decide.h, shared with the fit with camera offsets) one lane
//              per chain: the tiles' sums in ascending order (the same inputs give
//              the same bits), then mode 0: validity; mode 1: the seed's cost; mode 2: accept /
//              reject, mu, the stop tests, and which of the two state buffers holds the state (the
//              rules themselves are trajectory_fit_kernels.h's, shared with the skeleton fit).
//   solve_eliminate / _reduce / _backsub_kernel<FitSolveArgs>   the partition solver of
//              smooth_solver.h over the information-form buffer, the Marquardt factor (1 + mu_p) on
//              the diagonal entries; backsub writes the trial state X + δ into the chain's other
//              buffer.
//   fit_output_kernel<NoCoupling>   one lane per (t, p): out_xyz, Σ s² at the final state, the view
//              counts; per chain the costs and the status.
// mvp_trajectory_fit enqueues fit_run's sequence: prepare, sum, decide(0), terms<JAC>, sum,
// decide(1), then max_iter x (eliminate, reduce, backsub, terms at the trial, sum, decide(2),
// terms<JAC> at the state) and output.  A per-chain flag in the workspace makes a finished chain's
// lanes return at once, and a chain whose last trial was rejected keeps its linearisation.  Nothing
// is decided on the host.
//
// mvp_trajectory_fit_cov enqueues prepare, sum, decide(0) (the validity pass, at the given state),
// terms<JAC> at that state, then the three solver kernels over FitCovArgs: eliminate with no
// Marquardt factor and the pivots kept, reduce with the reduced system's selected inverse behind
// it, and the covariance sweep of smooth_solver.h.
//
// Register / LDS / scratch figures and the measurements are in DESIGN.md §4.14 and §4.16.
#include "trajectory_fit_decide.h"

// ------------------------------------------------------------------------------- host side

extern "C" int mvp_trajectory_fit_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks,
                                       int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const FitPlan pl = fit_plan("mvp_trajectory_fit_plan", T, P, chunk);
    if (chunk_used) *chunk_used = pl.sp.chunk;
    if (n_chunks) *n_chunks = pl.sp.n_chunks;
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_trajectory_fit_system(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                         const int* cam_idx, int n_cam_idx, const float* xyz, const uint8_t* mask,
                                         int weights, const double* gauss, float min_conf, float cov_floor,
                                         double huber_delta, double* out_H, double* out_g, uint8_t* out_nviews,
                                         double* out_cost, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_fit_system";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    MVP_REQUIRE(kpts && cams && xyz && out_H && out_g && out_nviews && out_cost, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    FitTerms a{};
    a.o = o;
    a.x32 = xyz;
    a.lambda = 1.0;
    a.H = out_H;
    a.g = out_g;
    a.nviews = out_nviews;
    hipLaunchKernelGGL((fit_terms_kernel<true, NoCoupling>), dim3(tri_grid(fn, (int64_t)T * P)), dim3(kBlock), 0, s, a,
                       NoCoupling{});
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_system_cost_kernel<NoCoupling>, dim3((unsigned)P), dim3(kBlock), 0, s, o, xyz, out_cost,
                       NoCoupling{});
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_trajectory_fit_cov_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks,
                                           int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const FitPlan pl = fit_plan("mvp_trajectory_fit_cov_plan", T, P, chunk);
    const CovPlan cp = cov_plan(pl.sp, P, pl.bytes);
    if (chunk_used) *chunk_used = pl.sp.chunk;
    if (n_chunks) *n_chunks = pl.sp.n_chunks;
    if (workspace_bytes) *workspace_bytes = cp.bytes;
    MVP_ABI_END
}

// prepare, sum, decide(0): the fit's validity pass at xyz; terms<JAC> at xyz: H̃; then eliminate
// (no Marquardt factor, pivots kept), reduce + its selected inverse, and the covariance sweep.
extern "C" int mvp_trajectory_fit_cov(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                      const int* cam_idx, int n_cam_idx, const float* xyz, const uint8_t* mask,
                                      int weights, const double* gauss, float min_conf, float cov_floor,
                                      double huber_delta, double lambda_smooth, int chunk, void* workspace,
                                      int64_t workspace_bytes, float* out_cov, float* out_cross, uint8_t* out_status,
                                      void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_fit_cov";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const FitPlan pl = fit_plan(fn, T, P, chunk);
    const CovPlan cp = cov_plan(pl.sp, P, pl.bytes);
    fit_check_args(fn, lambda_smooth, 0, 1.0, workspace_bytes, cp.bytes, T, P, 0, pl.sp.chunk);
    MVP_REQUIRE(kpts && cams && xyz && workspace && out_cov, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const FitChain ch = bind_chain(ws + pl.off_chain, P);
    double* x64 = reinterpret_cast<double*>(ws + pl.off_x);
    double* c2 = reinterpret_cast<double*>(ws + pl.off_cost);
    double* part = reinterpret_cast<double*>(ws + pl.off_part);
    FitCovArgs a{};
    bind_core(a, ws, pl.sp, T, P, lambda_smooth);
    bind_cov(a, ws, cp, out_cov, out_cross);
    a.H = reinterpret_cast<double*>(ws + pl.off_H);
    a.g = reinterpret_cast<double*>(ws + pl.off_g);
    a.invalid = ch.done;
    a.out_status = out_status;
    FitTerms ta{};
    ta.o = o;
    ta.x32 = xyz;   // the given state itself: no chain flag is read
    ta.lambda = lambda_smooth;
    ta.H = reinterpret_cast<double*>(ws + pl.off_H);
    ta.g = reinterpret_cast<double*>(ws + pl.off_g);
    const dim3 flat(tri_grid(fn, (int64_t)T * P)), blk(kBlock);
    const dim3 chain_grid((unsigned)((P + kSmBlock - 1) / kSmBlock)), lane_grid((unsigned)pl.sp.n_blocks), sm_blk(kSmBlock);
    MVP_HIP(hipMemsetAsync(a.cnt, 0, (size_t)P * 8, s));
    hipLaunchKernelGGL(fit_prepare_kernel<2>, flat, blk, 0, s, o, xyz, x64, c2);
    MVP_HIP(hipGetLastError());
    fit_launch_sum<2>(s, pl, c2, T, P, nullptr, part);
    hipLaunchKernelGGL(fit_decide_kernel, chain_grid, sm_blk, 0, s, ch, part, pl.n_tiles, P, 0, 0, 1.0, a.bad);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL((fit_terms_kernel<true, NoCoupling>), flat, blk, 0, s, ta, NoCoupling{});
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(solve_eliminate_kernel<FitCovArgs>, lane_grid, sm_blk, 0, s, a);
    hipLaunchKernelGGL(solve_reduce_kernel<FitCovArgs>, chain_grid, sm_blk, 0, s, a);
    hipLaunchKernelGGL(solve_backsub_kernel<FitCovArgs>, lane_grid, sm_blk, 0, s, a);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_trajectory_fit(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                  const int* cam_idx, int n_cam_idx, const float* xyz0, const uint8_t* mask,
                                  int weights, const double* gauss, float min_conf, float cov_floor,
                                  double huber_delta, double lambda_smooth, int max_iter, double tol, int chunk,
                                  void* workspace, int64_t workspace_bytes, float* out_xyz, float* out_resid,
                                  uint8_t* out_nviews, double* out_cost, uint8_t* out_status, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_fit";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const FitPlan pl = fit_plan(fn, T, P, chunk);
    fit_check_args(fn, lambda_smooth, max_iter, tol, workspace_bytes, pl.bytes, T, P, 0, pl.sp.chunk);
    MVP_REQUIRE(kpts && cams && xyz0 && workspace && out_xyz, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    fit_run(
        fn, s, pl, static_cast<char*>(workspace), o, NoCoupling{}, lambda_smooth, xyz0, max_iter,
        [&](int mode, const FitChain& ch, const double* part, int* bad) {
            hipLaunchKernelGGL(fit_decide_kernel, dim3((unsigned)((P + kSmBlock - 1) / kSmBlock)), dim3(kSmBlock), 0, s, ch,
                               part, pl.n_tiles, P, mode, max_iter, tol, bad);
        },
        [&](dim3 flat, dim3 blk, const FitChain& ch, const double* x64) {
            hipLaunchKernelGGL(fit_output_kernel<NoCoupling>, flat, blk, 0, s, o, xyz0, x64, ch, out_xyz, out_resid,
                               out_nviews, out_cost, out_status, NoCoupling{});
        });
    MVP_ABI_END
}

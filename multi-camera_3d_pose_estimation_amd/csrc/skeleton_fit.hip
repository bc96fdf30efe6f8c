// The trajectory fit with a person's joints coupled by bone lengths (mvp_skeleton_fit_plan /
// _system / mvp_skeleton_fit; the problem is stated in include/mvpose.h; the reference has the
// term in its Adam loop only, mvp_sgd_refine) for gfx950.
//
// P = G·J chains, chain p = g·J + j the joint j of person (group) g.  Per group, Levenberg-Marquardt
// on
//   f_g = Σ_chains (Σ_t Σ_used rho + ½ λ Σ_t |second difference|²) + ½ β Σ_t Σ_s (r − L_{g,s})²,
// r the distance of segment s's two joints in frame t.  The bone term enters a chain's frame block
// with its exact gradient and with 2β·[n nᵀ + max(0, 1 − L/r)·(I − n nᵀ)] on both ends, the a-b
// cross block dropped: a trial is then one block-pentadiagonal solve per chain, exactly the
// trajectory fit's (smooth_solver.h over trajectory_fit_solver.h's frame source), and the coupling
// acts from trial to trial.
//
// The kernels and the launch sequence are the trajectory fit's, trajectory_fit_kernels.h's, with
// the coupling policy of this file, SkBones, where the trajectory fit has none: it adds the bone
// terms (bone_terms) to a frame's, a third cost per frame, and r − L to the outputs.  What else
// differs is who decides: sk_decide_kernel, one workgroup per group, takes one mu, one accept /
// reject and one stop per group by the rules the trajectory fit applies per chain, and writes them
// to every chain of the group, so that the solver kernels run unchanged:
//
//   fit_terms_kernel<JAC, SkBones>   lanes along p, so that a frame's joints sit side by side: the
//              trajectory fit's terms plus, over the live segments that end at the lane's joint, the
//              other end's state (same frame, same buffer), the gradient and the curvature; the
//              segment's cost at its end a only.  Writes three cost terms per frame (Σ rho or +inf,
//              the prior's row, the bones).
//   sk_decide_kernel   lane j the joint j: the chain's tiles in ascending order, then lane 0 adds
//              the chains in ascending order (the same inputs give the same bits) and decides; every
//              lane writes the decision to its chain.  mode 0: validity of the chains; mode 1: the
//              group's cost at the seed; mode 2: accept / reject, mu, the stops.
//   fit_output_kernel<SkBones>   besides the trajectory fit's per-frame outputs, r − L of the
//              segments whose end a the lane is; per group the costs and the status.
// A segment is dead when its length is not finite or not > 0 or one of its chains is invalid; the
// segment table (at most 64 pairs) travels in the kernel arguments and is read by scalar loads, the
// loop over it is uniform.
//
// Register / LDS / scratch figures and the measurements are in DESIGN.md §4.15.
#include "trajectory_fit_kernels.h"

namespace {

constexpr int kSkMaxSeg = 64;
constexpr int kSkMaxJoints = 255;
constexpr int kSkGroupBlock = 256;   // the decide kernel's lanes: one per joint of the group

struct SkSegs {
    uint8_t a[kSkMaxSeg], b[kSkMaxSeg];
    int n, J;
    const float* len;   // [G][n]
    double beta;
};

// The per-group state of a fit, all [G] (kFitGroupBytes of the plan each).
struct SkGroup {
    double* mu;
    double* f;        // the state's cost
    double* fseed;
    double* bone;     // its bone part
    double* bseed;
    int* status;      // the group's status byte
    int* done;
};
static_assert(kFitGroupBytes == 5 * sizeof(double) + 2 * sizeof(int), "the plan's group block holds an SkGroup entry");

// The bone terms of joint j of person g at X: over the live segments that end at j, with Y the
// other end (other(jo, Y) loads it), d = X − Y, r = |d|, u = d / r (n or −n: the terms are even in
// it): g += β·(r − L)·u, H += 2β·[u uᵀ + max(0, 1 − L/r)·(I − u uᵀ)], nothing when r == 0.  Returns
// ½ Σ (r − L)² over the segments whose end a is j.  status: the chains' status (a segment to an
// invalid chain is dead) or null (every segment with a live length is live).
template <bool JAC, class Other>
__device__ __forceinline__ double bone_terms(const SkSegs& sg, int g, int j, const int* __restrict__ status,
                                             const double (&X)[3], Other other, double (&H)[6], double (&gr)[3]) {
#pragma clang fp contract(fast)
    double cb = 0.0;
#pragma unroll 1
    for (int s = 0; s < sg.n; s++) {
        const int a = sg.a[s], b = sg.b[s];
        if (a != j && b != j) continue;
        const int jo = a == j ? b : a;
        const float Lf = sg.len[(int64_t)g * sg.n + s];
        bool live = isfinite(Lf) && Lf > 0.f;
        if (status) live = live && status[g * sg.J + jo] != 0x80;
        if (!live) continue;
        const double L = (double)Lf;
        double Y[3];
        other(jo, Y);
        const double d0 = X[0] - Y[0], d1 = X[1] - Y[1], d2 = X[2] - Y[2];
        const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double e = r - L;
        if (a == j) cb += 0.5 * e * e;
        if (JAC && r != 0.0) {
            const double ir = 1.0 / r;
            const double u0 = d0 * ir, u1 = d1 * ir, u2 = d2 * ir;
            const double w = fmax(0.0, 1.0 - L * ir);
            const double c = 2.0 * sg.beta, cu = c * (1.0 - w), cw = c * w, ge = sg.beta * e;
            H[0] += cu * u0 * u0 + cw;
            H[1] += cu * u0 * u1;
            H[2] += cu * u0 * u2;
            H[3] += cu * u1 * u1 + cw;
            H[4] += cu * u1 * u2;
            H[5] += cu * u2 * u2 + cw;
            gr[0] += ge * u0;
            gr[1] += ge * u1;
            gr[2] += ge * u2;
        }
    }
    return cb;
}

// The coupling policy of trajectory_fit_kernels.h: the segments, and what the output kernel writes
// for them (null in the other kernels' copy).
struct SkBones {
    static constexpr int kCosts = 3;
    using Item = int64_t;
    SkSegs sg;
    SkGroup gr;
    float* out_bone;        // [T][G][n_seg] or null
    uint8_t* out_gstatus;   // [G] or null

    __device__ __forceinline__ int joints() const { return sg.J; }

    __device__ __forceinline__ double weight() const { return sg.beta; }

    // the bone terms of joint j of group g in frame e; a group's chains lie side by side
    template <bool JAC, class Other>
    __device__ __forceinline__ double frame_terms(int64_t e, int g, int j, const int* __restrict__ status,
                                                  const double (&X)[3], Other other, FitFrame& f) const {
#pragma clang fp contract(fast)
        const int64_t e0 = e - j;
        return bone_terms<JAC>(sg, g, j, status, X, [&](int jo, double (&Y)[3]) { other(e0 + jo, Y); }, f.H, f.g);
    }

    // r − L of the segments whose end a this joint is: every (t, g, s) is written by exactly one lane
    __device__ __forceinline__ void output_frame(const FitObs& o, const FitChain& ch, const double* __restrict__ x64,
                                                 int64_t buf, int64_t e, int t, int g, int j, bool valid,
                                                 const double (&X)[3]) const {
#pragma clang fp contract(fast)
        if (!out_bone) return;
        const int G = o.P / sg.J;
        const int64_t e0 = e - j;
#pragma unroll 1
        for (int s = 0; s < sg.n; s++) {
            if (sg.a[s] != j) continue;
            const int jo = sg.b[s];
            const float Lf = sg.len[(int64_t)g * sg.n + s];
            const bool live = valid && isfinite(Lf) && Lf > 0.f && ch.status[g * sg.J + jo] != 0x80;
            float v = __builtin_nanf("");
            if (live) {
                const double* yp = x64 + 3 * (buf + e0 + jo);
                const double d0 = X[0] - yp[0], d1 = X[1] - yp[1], d2 = X[2] - yp[2];
                v = (float)(sqrt(d0 * d0 + d1 * d1 + d2 * d2) - (double)Lf);
            }
            out_bone[((int64_t)t * G + g) * sg.n + s] = v;
        }
    }

    // out_cost [G][4]: the seed's cost, the state's, and the bone part of each; out_status [P]
    __device__ __forceinline__ void output_chain(const FitChain&, int p, int g, int j, int status,
                                                 double* __restrict__ out_cost, uint8_t* __restrict__ out_status) const {
        if (out_status) out_status[p] = status != 0x80 ? 0 : 0x80;
        if (j == 0) {
            if (out_cost) {
                out_cost[4 * g + 0] = gr.fseed[g];
                out_cost[4 * g + 1] = gr.f[g];
                out_cost[4 * g + 2] = gr.bseed[g];
                out_cost[4 * g + 3] = gr.bone[g];
            }
            if (out_gstatus) out_gstatus[g] = (uint8_t)gr.status[g];
        }
    }
};

// ------------------------------------------------------------------------------- decide
// mode 0: the chains' validity from prepare's sums; mode 1: the group's cost at the seed; mode 2:
// the trial's.  Lane j is chain g·J + j; lanes past J only keep the barriers.
__global__ __launch_bounds__(kSkGroupBlock) void sk_decide_kernel(FitChain ch, SkGroup gr,
                                                                  const double* __restrict__ part, int n_tiles, int P,
                                                                  int J, int mode, int max_iter, double tol,
                                                                  int* __restrict__ bad) {
    __shared__ double s_f[kSkGroupBlock], s_b[kSkGroupBlock];
    __shared__ int s_flag[kSkGroupBlock];
    __shared__ int s_dec[4];       // mode 1: the seed is finite; 2: accept, done
    __shared__ double s_mu;
    const int g = blockIdx.x, j = threadIdx.x;
    if (mode == 2 && gr.done[g]) return;   // the whole workgroup
    const int p = g * J + j;
    const bool mine = j < J;
    // a chain takes part once it is valid: decided in mode 0, from everybody's sums
    const bool part_of = mine && (mode == 0 || ch.status[p] != 0x80);
    double s[3] = {0.0, 0.0, 0.0};
    if (part_of) {
        fit_sum_tiles(part, n_tiles, P, p, s);
        bad[p] = 0;
    }
    if (mode == 0) {
        const bool valid = mine && fit_chain_valid(s[0], s[1]);
        s_flag[j] = valid ? 1 : 0;
        __syncthreads();
        if (j == 0) {
            int any = 0;
            for (int q = 0; q < J; q++) any |= s_flag[q];
            gr.mu[g] = 1e-3;
            gr.f[g] = gr.fseed[g] = gr.bone[g] = gr.bseed[g] = __builtin_nan("");
            gr.status[g] = any ? 0x40 : 0x80;
            gr.done[g] = any ? 0 : 1;
        }
        if (mine) fit_chain_reset(ch, p, valid, 0);
        return;
    }
    s_f[j] = s[0] + s[1];
    s_b[j] = s[2];
    s_flag[j] = part_of ? (mode == 2 && ch.rej[p] ? 3 : 1) : 0;   // bit 0: takes part; bit 1: a pivot failed
    __syncthreads();
    if (j == 0) {
        // the chains in ascending order, then the bones
        double F = 0.0, B = 0.0;
        int any = 0, rej = 0;
        for (int q = 0; q < J; q++) {
            if (!(s_flag[q] & 1)) continue;
            any = 1;
            rej |= s_flag[q] >> 1;
            F += s_f[q];
            B += s_b[q];
        }
        const double ft = F + B;
        if (mode == 1) {
            const bool fin = any && fit_seed_ok(ft);
            gr.f[g] = gr.fseed[g] = fin ? ft : __builtin_nan("");
            gr.bone[g] = gr.bseed[g] = fin ? B : __builtin_nan("");
            gr.status[g] = fin ? 0x40 : 0x80;
            gr.done[g] = (fin && max_iter > 0) ? 0 : 1;
            s_dec[0] = fin ? 1 : 0;
        } else {
            const LmStep st = lm_step(gr.f[g], ft, rej != 0, gr.mu[g], gr.status[g], max_iter, tol);
            if (st.accept) {
                gr.f[g] = ft;
                gr.bone[g] = B;
            }
            gr.mu[g] = st.mu;
            gr.status[g] = st.status;
            gr.done[g] = st.done ? 1 : 0;
            s_dec[0] = st.accept ? 1 : 0;
            s_dec[1] = st.done ? 1 : 0;
            s_mu = st.mu;
        }
    }
    __syncthreads();
    if (!part_of) return;
    if (mode == 1) {
        const bool fin = s_dec[0] != 0;
        ch.done[p] = (fin && max_iter > 0) ? 0 : 1;
        ch.status[p] = fin ? 0 : 0x80;   // the chains of an invalid group are returned as they came
        ch.relin[p] = 0;                 // the seed has just been linearised
        return;
    }
    const bool accept = s_dec[0] != 0;
    if (accept) ch.cur[p] ^= 1;
    ch.mu[p] = s_mu;
    ch.relin[p] = accept ? 1 : 0;
    ch.done[p] = s_dec[1];
}

// ------------------------------------------------------------------------------- host side
inline void sk_check_joints(const char* fn, int P, int J) {
    MVP_REQUIRE(J >= 1 && J <= kSkMaxJoints, "%s: J=%d (1..%d)", fn, J, kSkMaxJoints);
    MVP_REQUIRE(P % J == 0, "%s: P=%d is not a multiple of J=%d", fn, P, J);
}

// The segment arguments' checks; returns the table the kernels take.
inline SkSegs sk_parse(const char* fn, int P, int J, const int* seg, int n_seg, const float* seg_len,
                       double lambda_bone) {
    sk_check_joints(fn, P, J);
    MVP_REQUIRE(n_seg >= 0 && n_seg <= kSkMaxSeg, "%s: n_seg=%d (0..%d)", fn, n_seg, kSkMaxSeg);
    MVP_REQUIRE(n_seg == 0 || seg != nullptr, "%s: seg_host is NULL with n_seg=%d", fn, n_seg);
    MVP_REQUIRE(std::isfinite(lambda_bone) && lambda_bone >= 0, "%s: lambda_bone=%g must be finite and >= 0", fn,
                lambda_bone);
    SkSegs sg{};
    for (int s = 0; s < n_seg; s++) {
        const int a = seg[2 * s], b = seg[2 * s + 1];
        MVP_REQUIRE(a >= 0 && a < J && b >= 0 && b < J && a != b, "%s: seg_host[%d]=(%d, %d): two different joints below J=%d",
                    fn, s, a, b, J);
        for (int q = 0; q < s; q++)
            MVP_REQUIRE(!((sg.a[q] == a && sg.b[q] == b) || (sg.a[q] == b && sg.b[q] == a)),
                        "%s: seg_host[%d] repeats the pair of seg_host[%d]", fn, s, q);
        sg.a[s] = (uint8_t)a, sg.b[s] = (uint8_t)b;
    }
    MVP_REQUIRE(n_seg == 0 || seg_len != nullptr, "%s: seg_len_dev is NULL with n_seg=%d", fn, n_seg);
    sg.n = n_seg, sg.J = J, sg.len = seg_len, sg.beta = lambda_bone;
    return sg;
}

// The trajectory fit's plan with three costs per frame and a block of P / J groups; T, P and chunk
// are refused before J (a J below 1 plans no groups and is refused right after).
inline FitPlan sk_plan(const char* fn, int T, int P, int J, int chunk) {
    const FitPlan pl = fit_plan(fn, T, P, chunk, SkBones::kCosts, J >= 1 ? P / J : 0);
    sk_check_joints(fn, P, J);
    return pl;
}

// The groups' state in the plan's group block c.
inline SkGroup sk_bind_group(char* c, int G) {
    SkGroup gr;
    gr.mu = reinterpret_cast<double*>(c);
    gr.f = gr.mu + G;
    gr.fseed = gr.f + G;
    gr.bone = gr.fseed + G;
    gr.bseed = gr.bone + G;
    gr.status = reinterpret_cast<int*>(gr.bseed + G);
    gr.done = gr.status + G;
    return gr;
}

}  // namespace

extern "C" int mvp_skeleton_fit_plan(int T, int P, int J, int chunk, int* chunk_used, int* n_chunks,
                                     int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const FitPlan pl = sk_plan("mvp_skeleton_fit_plan", T, P, J, chunk);
    if (chunk_used) *chunk_used = pl.sp.chunk;
    if (n_chunks) *n_chunks = pl.sp.n_chunks;
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_skeleton_fit_system(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                       const int* cam_idx, int n_cam_idx, const float* xyz, const uint8_t* mask,
                                       int weights, const double* gauss, float min_conf, float cov_floor,
                                       double huber_delta, int J, const int* seg_host, int n_seg,
                                       const float* seg_len, double lambda_bone, double* out_H, double* out_g,
                                       uint8_t* out_nviews, double* out_cost, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_skeleton_fit_system";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    SkBones cp{};
    cp.sg = sk_parse(fn, P, J, seg_host, n_seg, seg_len, lambda_bone);
    MVP_REQUIRE(kpts && cams && xyz && out_H && out_g && out_nviews && out_cost, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    FitTerms a{};
    a.o = o;
    a.x32 = xyz;
    a.lambda = 1.0;
    a.H = out_H;
    a.g = out_g;
    a.nviews = out_nviews;
    hipLaunchKernelGGL((fit_terms_kernel<true, SkBones>), dim3(tri_grid(fn, (int64_t)T * P)), dim3(kBlock), 0, s, a, cp);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_system_cost_kernel<SkBones>, dim3((unsigned)(P / J)), dim3(kBlock), 0, s, o, xyz, out_cost, cp);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_skeleton_fit(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                const int* cam_idx, int n_cam_idx, const float* xyz0, const uint8_t* mask, int weights,
                                const double* gauss, float min_conf, float cov_floor, double huber_delta,
                                double lambda_smooth, int J, const int* seg_host, int n_seg, const float* seg_len,
                                double lambda_bone, int max_iter, double tol, int chunk, void* workspace,
                                int64_t workspace_bytes, float* out_xyz, float* out_resid, uint8_t* out_nviews,
                                float* out_bone, double* out_cost, uint8_t* out_group_status,
                                uint8_t* out_chain_status, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_skeleton_fit";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const FitPlan pl = sk_plan(fn, T, P, J, chunk);
    SkBones cp{};
    cp.sg = sk_parse(fn, P, J, seg_host, n_seg, seg_len, lambda_bone);
    fit_check_args(fn, lambda_smooth, max_iter, tol, workspace_bytes, pl.bytes, T, P, J, pl.sp.chunk);
    MVP_REQUIRE(kpts && cams && xyz0 && workspace && out_xyz, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const int G = P / J;
    cp.gr = sk_bind_group(ws + pl.off_group, G);
    cp.out_bone = out_bone;
    cp.out_gstatus = out_group_status;
    fit_run(
        fn, s, pl, ws, o, cp, lambda_smooth, xyz0, max_iter,
        [&](int mode, const FitChain& ch, const double* part, int* bad) {
            hipLaunchKernelGGL(sk_decide_kernel, dim3((unsigned)G), dim3(kSkGroupBlock), 0, s, ch, cp.gr, part, pl.n_tiles, P,
                               J, mode, max_iter, tol, bad);
        },
        [&](dim3 flat, dim3 blk, const FitChain& ch, const double* x64) {
            hipLaunchKernelGGL(fit_output_kernel<SkBones>, flat, blk, 0, s, o, xyz0, x64, ch, out_xyz, out_resid, out_nviews,
                               out_cost, out_chain_status, cp);
        });
    MVP_ABI_END
}

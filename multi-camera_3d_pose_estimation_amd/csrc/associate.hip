// Cross-view association of 2D skeletons (mvp_associate_views; the problem is stated in
// include/mvpose.h; no reference counterpart: the reference handles one person) for gfx950.
//
// Per frame, every (view, slot) skeleton is a node; nodes of different views are scored by the
// mean truncated squared Sampson distance of their common joints and grouped by complete-linkage
// agglomeration under the rule that a group holds at most one node per view.  Three stream-ordered
// launches, arithmetic in fp64:
//
//   fundamental, undistort   sync_common.h, as for mvp_epipolar_lag_cost: F_ab of every pair of
//                listed views, and the f32 undistorted pixel of every keypoint (NaN = not usable)
//                into a workspace plane [view][(frame·P + slot)·J + joint] of float2.
//   associate    one wavefront (a 64-lane workgroup) per frame, lane = node n = view·P + slot.
//                LDS holds the N x N link matrix (row stride N | 1 doubles, so that a row and a
//                column are both read without bank conflicts), the F matrices and, when they fit
//                beside them in 63 KiB, the frame's undistorted pixels (otherwise they are read
//                from the workspace: N = 64 with more than 57 joints).
//                  affinity  the (pair, slot a, slot b) entries, in the order of the affinity
//                            output, are dealt to the lanes 64 at a time: each unordered node pair
//                            is computed once and written to both halves of the matrix.
//                  merge     at most N − 1 rounds.  A live lane is its cluster's smallest node and
//                            keeps the cluster's best partner with a larger node number.  A row is
//                            scanned by all lanes at once (lane m offers link[r][m]; a butterfly
//                            minimum and a ballot for the lowest lane that holds it).  Per round:
//                            the wave's smallest (link, node a, node b) the same way, row and
//                            column a become max(row a, row b) (undefined = −1), and only row a
//                            and the rows whose partner was a or b are scanned again: links only
//                            grow and admissible pairs only shrink, so every other partner stands.
//                  label     clusters are ranked by (−views, smallest node) through 64 ints in LDS.
// No atomics, one wave per frame: the same inputs give the same bits on every call.
//
// Register / LDS figures and the measurements are in DESIGN.md §4.11.
#pragma clang fp contract(off)

#include "sync_common.h"

#include <climits>

namespace {

constexpr int kAsWave = 64;
constexpr int kAsMaxJoints = 255;
constexpr int kAsLdsBudget = 63 * 1024;   // dynamic LDS of a workgroup: two fit in a CU's 160 KiB

struct AssocPlan {
    int N, ld, n_pairs, staged, lds_bytes;
    int64_t n, off_und, off_f, bytes;
};

inline AssocPlan assoc_plan(const char* fn, int T, int P, int J, int nv, float min_conf, float trunc_px,
                            float max_cost_px, int min_joints) {
    MVP_REQUIRE(T >= 1, "%s: T=%d < 1", fn, T);
    MVP_REQUIRE(nv >= 2 && nv <= kMaxCams, "%s: n_cam_idx=%d (2..%d)", fn, nv, kMaxCams);
    MVP_REQUIRE(P >= 1 && (int64_t)nv * P <= kAsWave, "%s: P=%d slots must satisfy 1 <= P, n_cam_idx*P=%lld <= %d", fn, P,
                (long long)nv * P, kAsWave);
    MVP_REQUIRE(J >= 1 && J <= kAsMaxJoints, "%s: J=%d (1..%d)", fn, J, kAsMaxJoints);
    MVP_REQUIRE((int64_t)T * P * J < (1LL << 31), "%s: T*P*J=%lld too large", fn, (long long)T * P * J);
    MVP_REQUIRE(!std::isnan(min_conf), "%s: min_conf is NaN", fn);
    MVP_REQUIRE(std::isfinite(trunc_px) && std::isfinite(max_cost_px) && max_cost_px > 0.f && max_cost_px < trunc_px,
                "%s: max_cost_px=%g, trunc_px=%g must be finite with 0 < max_cost_px < trunc_px", fn,
                (double)max_cost_px, (double)trunc_px);
    MVP_REQUIRE(min_joints >= 1 && min_joints <= J, "%s: min_joints=%d (1..J=%d)", fn, min_joints, J);
    AssocPlan pl;
    pl.N = nv * P;
    pl.ld = pl.N | 1;
    pl.n_pairs = nv * (nv - 1) / 2;
    pl.n = (int64_t)T * P * J;
    const int base = pl.N * pl.ld * 8 + pl.n_pairs * 72;
    const int px = pl.N * J * 8;
    pl.staged = base + px <= kAsLdsBudget;
    pl.lds_bytes = base + (pl.staged ? px : 0);
    int64_t b = 0;
    pl.off_und = b;
    b = sy_align256(b + (int64_t)nv * pl.n * 8);
    pl.off_f = b;
    b = sy_align256(b + (int64_t)pl.n_pairs * 9 * 8);
    pl.bytes = b;
    return pl;
}

struct AssocArgs {
    const float2* und;   // [nv][T·P·J]
    const double* fmat;  // [n_pairs][9]
    int8_t* group;       // [T][N]
    uint8_t* count;      // [T][2]
    double* aff;         // [T][n_pairs][P][P] or null
    int64_t n;           // T·P·J
    int P, J, nv, N, ld, n_pairs, min_joints;
    double tau2, thr2;
};

template <bool STAGED>
__global__ __launch_bounds__(kAsWave) void assoc_kernel(AssocArgs g) {
#pragma clang fp contract(fast)
    // [link N x ld | F n_pairs x 9 | pixels N x J when STAGED], every piece 8-byte aligned
    extern __shared__ __attribute__((aligned(16))) char as_smem[];
    __shared__ int s_key[kAsWave], s_rank[kAsWave];
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int N = g.N, P = g.P, J = g.J, ld = g.ld, nv = g.nv;
    const int PJ = P * J;
    double* link = reinterpret_cast<double*>(as_smem);
    double* sf = link + N * ld;
    float2* spx = reinterpret_cast<float2*>(sf + g.n_pairs * 9);
    const float2* gpx = g.und + t * PJ;     // view i's slot p, joint j: gpx[i·n + p·J + j]
    for (int e = lane; e < N * ld; e += kAsWave) link[e] = -1.0;
    for (int e = lane; e < g.n_pairs * 9; e += kAsWave) sf[e] = g.fmat[e];
    if (STAGED)
        for (int e = lane; e < N * J; e += kAsWave) {
            const int view = e / PJ;
            spx[e] = gpx[(int64_t)view * g.n + (e - view * PJ)];
        }
    __syncthreads();
    auto px = [&](int node, int j) -> float2 {
        if (STAGED) return spx[node * J + j];
        const int view = node / P;
        return gpx[(int64_t)view * g.n + (node - view * P) * J + j];
    };

    // a node is usable when min_joints of its keypoints are
    int n_usable = 0;
    if (lane < N)
        for (int j = 0; j < J; j++) n_usable += isnan(px(lane, j).x) ? 0 : 1;
    const bool usable = lane < N && n_usable >= g.min_joints;

    // affinity: entry q = (pair·P + slot a)·P + slot b, the layout of the optional output
    const int PP = P * P, E = g.n_pairs * PP;
    for (int q = lane; q < E; q += kAsWave) {
        const int pair = q / PP, r = q - pair * PP;
        const int sa = r / P, sb = r - sa * P;
        int a = 0, rem = pair;
        while (rem >= nv - 1 - a) {        // pair -> (a, b), lexicographic
            rem -= nv - 1 - a;
            a++;
        }
        const int na = a * P + sa, nb = (a + 1 + rem) * P + sb;
        const double* F = sf + 9 * pair;
        const double f00 = F[0], f01 = F[1], f02 = F[2], f10 = F[3], f11 = F[4], f12 = F[5], f20 = F[6], f21 = F[7],
                     f22 = F[8];
        double sum = 0.0;
        int cnt = 0;
        for (int j = 0; j < J; j++) {
            const float2 pa = px(na, j), pb = px(nb, j);
            const double xa = pa.x, ya = pa.y, xb = pb.x, yb = pb.y;
            const double l0 = f00 * xa + f01 * ya + f02, l1 = f10 * xa + f11 * ya + f12, l2 = f20 * xa + f21 * ya + f22;
            const double g0 = f00 * xb + f10 * yb + f20, g1 = f01 * xb + f11 * yb + f21;
            const double num = xb * l0 + yb * l1 + l2;
            const double den = (l0 * l0 + l1 * l1) + (g0 * g0 + g1 * g1);
            const double d2 = num * num * rcp_nr(den);
            const bool ok = den != 0.0 && __builtin_isfinite(d2);
            sum += ok ? (d2 < g.tau2 ? d2 : g.tau2) : 0.0;
            cnt += ok ? 1 : 0;
        }
        const double c = cnt >= g.min_joints ? sum / (double)cnt : -1.0;
        if (g.aff) g.aff[t * E + q] = c;
        link[na * ld + nb] = c;
        link[nb * ld + na] = c;
    }
    __syncthreads();

    // merge: a live lane is the smallest node of its cluster and keeps the cluster's best partner
    // among the live clusters with a larger node number (each pair is held by one lane)
    bool alive = usable;
    unsigned vmask = usable ? 1u << (lane / P) : 0u;
    int rep = lane;
    const double inf = __builtin_inf();
    double best = inf;
    int bj = 0;
    // the wave's minimum of v, the same value in every lane
    auto wave_min = [](double v) {
        for (int off = kAsWave / 2; off; off >>= 1) {
            const double o = __shfl_xor(v, off);
            v = o < v ? o : v;
        }
        return v;
    };
    // row r's best partner, by all lanes at once: lane m offers link[r][m]; ties to the smallest m
    auto rescan = [&](int r) {
        const unsigned vr = __shfl(vmask, r);
        double v = inf;
        if (alive && lane > r && (vmask & vr) == 0u) {
            const double l = link[r * ld + lane];
            v = (l >= 0.0 && l <= g.thr2) ? l : inf;
        }
        const double mn = wave_min(v);
        const unsigned long long at = __ballot(v < inf && v == mn);
        if (lane == r) {
            best = mn;
            bj = at ? __builtin_ctzll(at) : 0;
        }
    };
    for (unsigned long long rest = __ballot(alive); rest; rest &= rest - 1) rescan(__builtin_ctzll(rest));
    for (int round = 0; round + 1 < N; round++) {
        // the smallest (link, node a, node b): the smallest link, then the lowest lane that holds it
        const double mn = wave_min(best);
        if (!(mn < inf)) break;
        const int i = __builtin_ctzll(__ballot(best == mn));
        const int j = __builtin_amdgcn_readfirstlane(__shfl(bj, i));
        if (lane < N && lane != i && lane != j) {
            const double li = link[i * ld + lane], lj = link[j * ld + lane];
            const double mx = li > lj ? li : lj;
            link[i * ld + lane] = mx;
            link[lane * ld + i] = mx;
        }
        const unsigned vj = __shfl(vmask, j);
        if (lane == i) vmask |= vj;
        if (lane == j) {
            alive = false;
            best = inf;
        }
        if (rep == j) rep = i;
        __syncthreads();
        // links only grow and the admissible pairs only shrink: a cluster's best partner stands
        // unless it was i or j; cluster i starts over
        const unsigned long long redo = __ballot(alive && (lane == i || (best < inf && (bj == i || bj == j))));
        for (unsigned long long rest = redo; rest; rest &= rest - 1) rescan(__builtin_ctzll(rest));
    }

    // number the groups by (−views, smallest node)
    const int views = __builtin_popcount(vmask);
    const int key = alive ? (kMaxCams - views) * kAsWave + lane : INT_MAX;
    s_key[lane] = key;
    __syncthreads();
    int rank = 0;
    for (int m = 0; m < N; m++) rank += s_key[m] < key ? 1 : 0;
    s_rank[lane] = rank;
    __syncthreads();
    if (lane < N) g.group[t * N + lane] = usable ? (int8_t)s_rank[rep] : (int8_t)-1;
    const unsigned long long groups = __ballot(alive), multi = __ballot(alive && views >= 2);
    if (lane == 0) {
        g.count[2 * t] = (uint8_t)__builtin_popcountll(groups);
        g.count[2 * t + 1] = (uint8_t)__builtin_popcountll(multi);
    }
}

}  // namespace

extern "C" int mvp_associate_views_plan(int T, int P, int J, int n_cam_idx, float min_conf, float trunc_px,
                                        float max_cost_px, int min_joints, int* lds_bytes, int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const AssocPlan pl = assoc_plan("mvp_associate_views_plan", T, P, J, n_cam_idx, min_conf, trunc_px, max_cost_px,
                                    min_joints);
    if (lds_bytes) *lds_bytes = pl.lds_bytes;
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_associate_views(const float* kpts, int T, int P, int J, int V, const double* cams, int n_cams,
                                   const int* cam_idx, int n_cam_idx, float min_conf, float trunc_px,
                                   float max_cost_px, int min_joints, void* workspace, int64_t workspace_bytes,
                                   int8_t* out_group, uint8_t* out_count, double* out_affinity, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_associate_views";
    const AssocPlan pl = assoc_plan(fn, T, P, J, n_cam_idx, min_conf, trunc_px, max_cost_px, min_joints);
    const CamIdx ci = tri_parse_args(fn, pl.n, V, n_cams, cam_idx, n_cam_idx);
    MVP_REQUIRE(workspace_bytes >= pl.bytes, "%s: workspace_bytes=%lld < %lld needed (T=%d, P=%d, J=%d, n_cam_idx=%d)", fn,
                (long long)workspace_bytes, (long long)pl.bytes, T, P, J, n_cam_idx);
    MVP_REQUIRE(kpts && cams && workspace && out_group && out_count, "%s: null device pointer", fn);
    SyncPairs pr{};
    const int np = sync_list_pairs(n_cam_idx, pr);
    char* ws = static_cast<char*>(workspace);
    float2* und = reinterpret_cast<float2*>(ws + pl.off_und);
    double* fmat = reinterpret_cast<double*>(ws + pl.off_f);
    AssocArgs g{};
    g.und = und;
    g.fmat = fmat;
    g.group = out_group;
    g.count = out_count;
    g.aff = out_affinity;
    g.n = pl.n;
    g.P = P;
    g.J = J;
    g.nv = n_cam_idx;
    g.N = pl.N;
    g.ld = pl.ld;
    g.n_pairs = np;
    g.min_joints = min_joints;
    g.tau2 = (double)trunc_px * (double)trunc_px;
    g.thr2 = (double)max_cost_px * (double)max_cost_px;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sync_fundamental_kernel, dim3(1), dim3(64), 0, s, cams, ci, pr, np, fmat);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(sync_undistort_kernel, dim3(tri_grid(fn, pl.n), (unsigned)n_cam_idx), dim3(kBlock), 0, s, kpts,
                       pl.n, V, cams, n_cams, ci, min_conf, und);
    MVP_HIP(hipGetLastError());
    if (pl.staged)
        hipLaunchKernelGGL(assoc_kernel<true>, dim3((unsigned)T), dim3(kAsWave), (size_t)pl.lds_bytes, s, g);
    else
        hipLaunchKernelGGL(assoc_kernel<false>, dim3((unsigned)T), dim3(kAsWave), (size_t)pl.lds_bytes, s, g);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

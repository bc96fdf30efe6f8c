// Tracking of the triangulated groups through time (mvp_track_people; the rules are stated in
// include/mvpose.h; no reference counterpart: the reference handles one person) for gfx950.
//
// The problem is sequential in the frame but small per frame, so one wavefront (a 64-lane
// workgroup) walks one sequence from frame 0 to T − 1 inside a single launch; the M sequences are
// the grid.  LDS holds a ring of the last K + 1 = max_gap + 2 frames' joints and, per (ring slot,
// group), the track number of that observation while it is its track's latest one (−1 otherwise):
// a track is open exactly as long as its latest observation is still in the ring.  Per frame t:
//
//   prefetch   frame t + 1's joints are loaded into registers (8 floats per lane; what a larger
//              frame has beyond them is loaded when the slot is written), so that their latency is
//              spent under the stages below.
//   live       the K·G² combinations (lag k, group h of frame t − k, group g of frame t) are dealt
//              to the lanes 64 at a time, at most 16 per lane; which (k, h, g) a lane's entries
//              are never changes, so they are decoded once before the loop.  Few of them are live
//              (the observation open, the group present: about people² of them), and a single
//              wave pays for every instruction it issues, so the live ones are compacted, in
//              order, into a list in LDS (a ballot and a popcount below the lane per pass).
//   cost       live combination r belongs to lane r mod 64: it is scored in fp64 over the joints
//              finite in both (dx² + dy² + dz² is finite exactly then), six independent square
//              roots at a time, summed in joint order, and kept in a register when it is defined
//              and within its lag's limit.
//   link       at most G rounds: the wave's smallest (cost, k, h, g) by a butterfly over
//              (double, int) pairs that starts at the width the live list needs, the key's integer
//              being k·2¹⁶ + h·2⁸ + g; lane g takes the track, the entries of that g and of that
//              (k, h) are struck out of every lane.
//   close      the present groups left over number themselves by a popcount below their bit;
//              lanes 0..G−1 store the frame's outputs and its row of the track table, then the
//              prefetched frame replaces the oldest ring slot.
// No atomics, one wave per sequence, every loop bounded by T, G, J or K·G²: the same inputs give
// the same bits on every call.  Register / LDS figures and the measurements are in DESIGN.md §4.13.
#pragma clang fp contract(off)

#include "mvp_common.h"

#include <climits>
#include <cmath>
#include <cstdint>

namespace {

constexpr int kTrWave = 64;
constexpr int kTrMaxGroups = 8;
constexpr int kTrMaxGap = 15;
constexpr int kTrMaxJoints = 255;
constexpr int kTrMaxCand = kTrMaxGroups * kTrMaxGroups * (kTrMaxGap + 1) / kTrWave;   // 16 per lane
constexpr int kTrUnroll = 6;              // joint distances in flight per lane (17 joints: 6 + 6 + 5)
constexpr int kTrPrefetch = 8;            // floats of the next frame a lane holds in registers
constexpr int kTrLdsMax = 64 * 1024;

// ring [R][G][J][3] float, the track table [R][G] int32, the live list [K·G²] int32; R = K + 1 = max_gap + 2
inline int track_plan(const char* fn, int M, int T, int G, int J, int max_gap, float max_jump, float gap_growth,
                      int min_joints, bool check_params) {
    MVP_REQUIRE(M >= 1, "%s: M=%d < 1", fn, M);
    MVP_REQUIRE(T >= 1, "%s: T=%d < 1", fn, T);
    MVP_REQUIRE(G >= 1 && G <= kTrMaxGroups, "%s: G=%d (1..%d)", fn, G, kTrMaxGroups);
    MVP_REQUIRE(J >= 1 && J <= kTrMaxJoints, "%s: J=%d (1..%d)", fn, J, kTrMaxJoints);
    MVP_REQUIRE(max_gap >= 0 && max_gap <= kTrMaxGap, "%s: max_gap=%d (0..%d)", fn, max_gap, kTrMaxGap);
    if (check_params) {
        MVP_REQUIRE(std::isfinite(max_jump) && max_jump > 0.f, "%s: max_jump=%g must be finite and > 0", fn,
                    (double)max_jump);
        MVP_REQUIRE(std::isfinite(gap_growth) && gap_growth >= 0.f, "%s: gap_growth=%g must be finite and >= 0", fn,
                    (double)gap_growth);
        MVP_REQUIRE(min_joints >= 1 && min_joints <= J, "%s: min_joints=%d (1..J=%d)", fn, min_joints, J);
    }
    const int64_t mt = (int64_t)M * T;
    MVP_REQUIRE(mt < (1LL << 31) && mt * G * J < (1LL << 31), "%s: M*T*G*J=%lld*%d*%d too large (< 2^31)", fn,
                (long long)mt, G, J);
    const int lds = (max_gap + 2) * G * (J * 12 + 4) + (max_gap + 1) * G * G * 4;
    MVP_REQUIRE(lds <= kTrLdsMax,
                "%s: LDS %d bytes = (max_gap+2)*G*(12*J+4) + (max_gap+1)*G*G*4 with max_gap=%d, G=%d, J=%d exceeds %d", fn,
                lds, max_gap, G, J, kTrLdsMax);
    return lds;
}

struct TrackArgs {
    const float* xyz;      // [M][T][G][J][3]
    int32_t* track;        // [M][T][G]
    int32_t* n_tracks;     // [M]
    double* cost;          // [M][T][G] or null
    uint8_t* lag;          // [M][T][G] or null
    int T, G, J, K, min_joints;
    double max_jump, gap_growth;
};

// NC: the combinations a lane holds, K·G² <= 64·NC
template <int NC>
__global__ __launch_bounds__(kTrWave) void track_kernel(TrackArgs a) {
#pragma clang fp contract(fast)
    extern __shared__ __attribute__((aligned(16))) char tr_smem[];
    const int lane = threadIdx.x;
    const int T = a.T, G = a.G, J = a.J, K = a.K, R = K + 1;
    const int J3 = J * 3, GJ3 = G * J3, GG = G * G, E = K * GG;
    float* ring = reinterpret_cast<float*>(tr_smem);
    int* open = reinterpret_cast<int*>(ring + R * GJ3);
    int* live = open + R * G;
    const int64_t seq = blockIdx.x;
    const float* x = a.xyz + seq * T * GJ3;
    int32_t* out_track = a.track + seq * T * G;
    double* out_cost = a.cost ? a.cost + seq * T * G : nullptr;
    uint8_t* out_lag = a.lag ? a.lag + seq * T * G : nullptr;
    const double inf = __builtin_inf();
    const unsigned long long below = (1ull << lane) - 1ull;

    // this lane's combinations, k·2¹⁶ + h·2⁸ + g (ascending in the entry number), −1 beyond E
    int code[NC];
#pragma unroll
    for (int i = 0; i < NC; i++) {
        const int q = lane + kTrWave * i;
        const int k = q / GG, r = q - k * GG, h = r / G, g = r - h * G;
        code[i] = q < E ? ((k + 1) << 16) | (h << 8) | g : -1;
    }
    for (int e = lane; e < R * G; e += kTrWave) open[e] = -1;
    for (int e = lane; e < GJ3; e += kTrWave) ring[e] = x[e];
    __syncthreads();

    int n_tracks = 0;
    int slot = 0;                                   // t % R
    for (int t = 0; t < T; t++) {
        const bool more = t + 1 < T;
        const float* xn = x + (int64_t)(t + 1) * GJ3;
        float pf[kTrPrefetch];
#pragma unroll
        for (int i = 0; i < kTrPrefetch; i++) {
            const int e = lane + kTrWave * i;
            pf[i] = (more && e < GJ3) ? xn[e] : 0.f;
        }

        // present groups of frame t: lane = (joint phase, group), OR over the wave
        const float* cur = ring + slot * GJ3;
        unsigned present = 0;
        {
            const int g = lane & (kTrMaxGroups - 1);
            if (g < G)
                for (int j = lane / kTrMaxGroups; j < J; j += kTrWave / kTrMaxGroups) {
                    const float* p = cur + g * J3 + 3 * j;
                    const bool seen = __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]);
                    present |= seen ? 1u << g : 0u;
                }
            for (int off = kTrWave / 2; off; off >>= 1) present |= __shfl_xor(present, off);
        }

        // live: the combinations to score, in ascending (k, h, g)
        int n_live = 0;
#pragma unroll
        for (int i = 0; i < NC; i++)
            if (kTrWave * i < E) {
                const int cd = code[i];
                const int k = cd >> 16, h = (cd >> 8) & 0xff, g = cd & 0xff;
                bool is = cd >= 0 && k <= t && ((present >> g) & 1u);
                if (is) {
                    int sk = slot - k;
                    sk += sk < 0 ? R : 0;
                    is = open[sk * G + h] >= 0;
                }
                const unsigned long long m = __ballot(is);
                if (is) live[n_live + __builtin_popcountll(m & below)] = cd;
                n_live += __builtin_popcountll(m);
            }
        __syncthreads();

        // cost: a candidate keeps its cost, everything else is +inf
        double c[NC];
        int cc[NC];
#pragma unroll
        for (int i = 0; i < NC; i++) {
            c[i] = inf;
            cc[i] = INT_MAX;
            if (kTrWave * i < n_live) {
                const int r = lane + kTrWave * i;
                if (r < n_live) {
                    const int cd = live[r];
                    const int k = cd >> 16, h = (cd >> 8) & 0xff, g = cd & 0xff;
                    int sk = slot - k;
                    sk += sk < 0 ? R : 0;
                    const float* pa = cur + g * J3;
                    const float* pb = ring + sk * GJ3 + h * J3;
                    double sum = 0.0;
                    int cnt = 0;
                    // kTrUnroll independent distances at a time, then summed in joint order
                    for (int j0 = 0; j0 < J; j0 += kTrUnroll) {
                        double d[kTrUnroll];
#pragma unroll
                        for (int u = 0; u < kTrUnroll; u++) {
                            const int j = 3 * (j0 + u < J ? j0 + u : J - 1);    // past J: read in bounds, not counted
                            const double dx = (double)pa[j] - (double)pb[j], dy = (double)pa[j + 1] - (double)pb[j + 1],
                                         dz = (double)pa[j + 2] - (double)pb[j + 2];
                            const double d2 = dx * dx + dy * dy + dz * dz;      // finite = seen in both
                            d[u] = (j0 + u < J && __builtin_isfinite(d2)) ? sqrt(d2) : -1.0;
                        }
#pragma unroll
                        for (int u = 0; u < kTrUnroll; u++) {
                            sum += d[u] >= 0.0 ? d[u] : 0.0;
                            cnt += d[u] >= 0.0 ? 1 : 0;
                        }
                    }
                    const double limit = a.max_jump * (1.0 + a.gap_growth * (double)(k - 1));
                    const double v = sum / (double)cnt;
                    c[i] = (cnt >= a.min_joints && v <= limit) ? v : inf;
                    cc[i] = cd;
                }
            }
        }
        __syncthreads();            // the oldest slot, the table and the list have been read

        // link: the smallest (cost, k, h, g) of the wave, at most once per group.  The candidates sit
        // in lanes 0..min(64, n_live)−1: the butterfly starts at the power of two that covers them
        // and lane 0 ends up with the minimum.
        const int n_lanes = n_live < kTrWave ? n_live : kTrWave;
        const int top = n_lanes > 1 ? 1 << (31 - __builtin_clz(n_lanes - 1)) : 0;
        int my_track = -1, my_lag = 0;
        double my_cost = __builtin_nan("");
        unsigned taken = 0;
        for (int round = 0; round < G; round++) {
            double bc = inf;
            int bk = INT_MAX;
#pragma unroll
            for (int i = 0; i < NC; i++)
                if (kTrWave * i < n_live && c[i] < bc) {      // ascending i = ascending key within a lane
                    bc = c[i];
                    bk = cc[i];
                }
            if (__ballot(bc < inf) == 0ull) break;      // nothing left: no butterfly for it
            for (int off = top; off; off >>= 1) {
                const double oc = __shfl_xor(bc, off);
                const int ok = __shfl_xor(bk, off);
                if (oc < bc || (oc == bc && ok < bk)) {
                    bc = oc;
                    bk = ok;
                }
            }
            bc = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(bc)),
                                  __builtin_amdgcn_readfirstlane(__double2loint(bc)));
            bk = __builtin_amdgcn_readfirstlane(bk);
            const int k = bk >> 16, h = (bk >> 8) & 0xff, g = bk & 0xff;
            int sk = slot - k;
            sk += sk < 0 ? R : 0;
            const int tr = open[sk * G + h];
            if (lane == g) {
                my_track = tr;
                my_cost = bc;
                my_lag = k;
            }
            if (lane == 0) open[sk * G + h] = -1;       // no longer its track's latest observation
            taken |= 1u << g;
#pragma unroll
            for (int i = 0; i < NC; i++)
                if (kTrWave * i < n_live && ((cc[i] & 0xff) == g || (cc[i] >> 8) == (bk >> 8))) c[i] = inf;
        }

        // close: new tracks in ascending g, the frame's outputs and its row of the table
        const unsigned fresh = present & ~taken;
        if (lane < G) {
            if ((fresh >> lane) & 1u) my_track = n_tracks + __builtin_popcount(fresh & ((1u << lane) - 1u));
            out_track[(int64_t)t * G + lane] = my_track;
            if (out_cost) out_cost[(int64_t)t * G + lane] = my_cost;
            if (out_lag) out_lag[(int64_t)t * G + lane] = (uint8_t)my_lag;
            open[slot * G + lane] = my_track;
        }
        n_tracks += __builtin_popcount(fresh);
        const int ns = slot + 1 == R ? 0 : slot + 1;    // R >= 2: never the slot just closed
        if (more) {
            float* nxt = ring + ns * GJ3;
#pragma unroll
            for (int i = 0; i < kTrPrefetch; i++) {
                const int e = lane + kTrWave * i;
                if (e < GJ3) nxt[e] = pf[i];
            }
            for (int e = lane + kTrWave * kTrPrefetch; e < GJ3; e += kTrWave) nxt[e] = xn[e];
        }
        slot = ns;
        __syncthreads();
    }
    if (lane == 0) a.n_tracks[seq] = n_tracks;
}

}  // namespace

extern "C" int mvp_track_people_plan(int M, int T, int G, int J, int max_gap, int* lds_bytes) {
    MVP_ABI_BEGIN
    const int lds = track_plan("mvp_track_people_plan", M, T, G, J, max_gap, 1.f, 0.f, 1, false);
    if (lds_bytes) *lds_bytes = lds;
    MVP_ABI_END
}

extern "C" int mvp_track_people(const float* xyz, int M, int T, int G, int J, int max_gap, float max_jump,
                                float gap_growth, int min_joints, int32_t* out_track, int32_t* out_n_tracks,
                                double* out_link_cost, uint8_t* out_link_lag, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_track_people";
    const int lds = track_plan(fn, M, T, G, J, max_gap, max_jump, gap_growth, min_joints, true);
    MVP_REQUIRE(xyz && out_track && out_n_tracks, "%s: null device pointer", fn);
    TrackArgs a{};
    a.xyz = xyz;
    a.track = out_track;
    a.n_tracks = out_n_tracks;
    a.cost = out_link_cost;
    a.lag = out_link_lag;
    a.T = T;
    a.G = G;
    a.J = J;
    a.K = max_gap + 1;
    a.min_joints = min_joints;
    a.max_jump = (double)max_jump;
    a.gap_growth = (double)gap_growth;
    const int E = a.K * G * G;
    auto kern = E <= kTrWave ? track_kernel<1> : E <= 2 * kTrWave ? track_kernel<2> : E <= 4 * kTrWave ? track_kernel<4>
                : E <= 8 * kTrWave ? track_kernel<8> : track_kernel<kTrMaxCand>;
    hipLaunchKernelGGL(kern, dim3((unsigned)M), dim3(kTrWave), (size_t)lds, reinterpret_cast<hipStream_t>(stream), a);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

// The decide kernel of the fits whose chains stand alone (trajectory_fit.hip, trajectory_fit_lag.hip);
// the rules themselves are trajectory_fit_kernels.h's, shared with the skeleton fit, whose groups
// decide in a kernel of its own.
#pragma once
#include "trajectory_fit_kernels.h"

namespace {

// One lane per chain.  mode 0: validity from prepare's sums; mode 1: the seed's cost; mode 2: the trial's.
__global__ __launch_bounds__(kSmBlock) void fit_decide_kernel(FitChain ch, const double* __restrict__ part, int n_tiles,
                                                              int P, int mode, int max_iter, double tol,
                                                              int* __restrict__ bad) {
    const int p = blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    if (mode != 0 && ch.done[p]) return;
    double s[2];
    fit_sum_tiles(part, n_tiles, P, p, s);
    bad[p] = 0;
    if (mode == 0) {
        fit_chain_reset(ch, p, fit_chain_valid(s[0], s[1]), 0x40);
        return;
    }
    const double ft = s[0] + s[1];
    if (mode == 1) {
        const bool fin = fit_seed_ok(ft);
        ch.f[p] = ch.fseed[p] = fin ? ft : __builtin_nan("");
        ch.done[p] = (fin && max_iter > 0) ? 0 : 1;
        ch.status[p] = fin ? 0x40 : 0x80;
        ch.relin[p] = 0;   // the seed has just been linearised
        return;
    }
    const LmStep st = lm_step(ch.f[p], ft, ch.rej[p] != 0, ch.mu[p], ch.status[p], max_iter, tol);
    if (st.accept) {
        ch.cur[p] ^= 1;
        ch.f[p] = ft;
    }
    ch.mu[p] = st.mu;
    ch.relin[p] = st.accept ? 1 : 0;
    ch.status[p] = st.status;
    ch.done[p] = st.done ? 1 : 0;
}

}  // namespace

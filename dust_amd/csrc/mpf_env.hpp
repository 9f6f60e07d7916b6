// mpf_env.hpp - what a batched filter update reads per environment beside its particles: the observation pair, the action between them
// and the optimiser steps taken so far.  mpf_optimize_batch_kernel (mpf.hpp) reads the rows; the host stages them per call
// (mpfb_enqueue), or svmpc_dual_period_kernel (svmpc_episode.hpp) conditions them on the device, period after period.
#pragma once

namespace dust {

struct MpfEnvIn {
  float past_obs[4], obs[4], past_action[2];
  int t0, pad;
};

}  // namespace dust

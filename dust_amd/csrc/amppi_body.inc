// amppi_body.inc - the statements of the AMPPI tick's kernel (amppi.hpp has the account), included TEXTUALLY into each kernel that runs
// them: amppi_kernel<MODEL>, amppi_skid_nav_kernel, their PRIOR and their batched forms.  Text, not a function: hipcc schedules the plain instances differently once their
// body is an inlined callee, and they are to stay the instructions they were.  In scope at the point of inclusion:
//   MODEL (int), NAV (constexpr bool), a (const AmppiArgs &; the batched kernels: AmppiEnvArgs, one environment's view with the same member
//   names), nav (const SkidNav *, NAV only), grid_lds (uint32_t *: dynamic LDS, NAV only)
//   PRIOR (constexpr bool), pri (const AmppiPrior *, PRIOR only): the lane draws its own parameter row from the filter's prior
// The static __shared__ object below is declared once per including kernel; the NAV kernel's dynamic LDS lies behind it.
// BEFORE turning this text into a function (or moving a declaration out of it): build both ways for gfx950 and compare the disassembly and
// the register metadata of the four amppi_kernel instances - as a force-inlined callee they came out 2-3 instructions longer, with another
// induction variable in the Philox loop and another SGPR allocation (DESIGN.md section 7).  Convert only if they come out the same.
  constexpr int DS = AmppiDims<MODEL>::DS;
  // ONE LDS object: [0] "this workgroup is the reducer", [1, 9) block_reduce's scratch, [9, 13) wave partials, [16, 16 + 256) column partials
  __shared__ double lds[16 + AMPPI_THREADS];
  DevModel map_store;  // (NAV only: dead in the plain instances)
  const DevModel *map = nullptr;
  if constexpr (NAV) {
    map_store = skid_nav_map(*nav, grid_lds);
    map = &map_store;
  }
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x * AMPPI_THREADS + tid;
  const int D = a.D, H = a.H, da = a.da, S = a.S;

  if (s < S) {
    float *acts = a.acts + (size_t)s * D;
    if (a.philox) {
      const uint32_t ctr_tick = a.ctr[0], ctr_iter = a.ctr[1];
      for (int j0 = 0; j0 < D; j0 += 8) {
        float z[8];
        philox_normal8(a.seed, (uint32_t)(j0 >> 3), (uint32_t)s, ctr_iter, ctr_tick, z);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int j = j0 + i;
          if (j >= D) break;
          // a_seq + L z: an odd column of a 2 x 2 factor takes its partner draw too (D is even then: pairs never straddle a block)
          const float lz = (da == 2 && (i & 1)) ? (a.chol[1] * z[i - 1] + a.chol[2] * z[i]) : a.chol[0] * z[i];
          acts[j] = a.a_seq[j] + lz;
        }
      }
    }
    double cc = 0.0;
    for (int t = 0; t < H; ++t) {
      if (da == 1) {
        const float e0 = acts[t] - a.a_seq[t];
        cc += (double)((a.a_seq[t] * a.pre[0]) * e0);
      } else {
        const float u0 = a.a_seq[2 * t], u1 = a.a_seq[2 * t + 1];
        const float e0 = acts[2 * t] - u0, e1 = acts[2 * t + 1] - u1;
        const float p0 = u0 * a.pre[0] + u1 * a.pre[1], p1 = u0 * a.pre[1] + u1 * a.pre[2];
        cc += (double)(p0 * e0 + p1 * e1);
      }
    }
    const float ctrl = a.lambda * (float)cc;
    float inst = 0.f, term = 0.f;
    if constexpr (PRIOR) {
      // row s of mpf.prior.sample([S]) as mpf_sample_kernel (mpf.hpp) draws it: the same counters, the same operations in the same order
      uint32_t r[4];
      philox4x32_10((uint32_t)s, 0x6d7066u, 0u, 0u, (uint32_t)pri->seed, (uint32_t)(pri->seed >> 32), r);
      const int kc = (int)(((unsigned long long)r[0] * (unsigned long long)pri->K) >> 32);
      float zp[4], row[4];
      philox_normal4(pri->seed, (uint32_t)s, 0x6d7067u, 1u, 0u, zp);
#pragma unroll
      for (int p = 0; p < 4; ++p) row[p] = p < pri->P ? pri->means[kc * pri->P + p] + pri->bw[p] * zp[p] : 0.f;
      if (pri->params_out)
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (p < pri->P) pri->params_out[(size_t)s * pri->P + p] = row[p];
      float *so = a.states_out ? a.states_out + (size_t)s * (size_t)(H + 1) * DS : nullptr;
      amppi_traj<MODEL, NAV, true>(a, acts, row, so, &inst, &term, nav, map);
    } else if (a.mode == AMPPI_PARAMS_SIGMA) {
      double wi = 0.0, wt = 0.0;
      for (int k = 0; k < a.pts; ++k) {
        float ik, tk;
        float *so = a.states_out ? a.states_out + ((size_t)s * a.pts + k) * (size_t)(H + 1) * DS : nullptr;
        amppi_traj<MODEL, NAV>(a, acts, a.params + (size_t)k * a.P, so, &ik, &tk, nav, map);
        wi += (double)a.mw[k] * (double)ik;
        wt += (double)a.mw[k] * (double)tk;
      }
      inst = (float)wi;
      term = (float)wt;
    } else {
      const float *prow = a.mode == AMPPI_PARAMS_NONE ? nullptr : (a.mode == AMPPI_PARAMS_SINGLE ? a.params : a.params + (size_t)s * a.P);
      float *so = a.states_out ? a.states_out + (size_t)s * (size_t)(H + 1) * DS : nullptr;
      amppi_traj<MODEL, NAV>(a, acts, prow, so, &inst, &term, nav, map);
    }
    a.costs[s] = (term + inst) + ctrl;  // amppi.py:224
  }

  // ---- publish, take a ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  wg_sync();
  unsigned int *is_last = reinterpret_cast<unsigned int *>(lds);
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned int last = t + 1u == gridDim.x ? 1u : 0u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *is_last = last;
  }
  wg_sync();
  if (*is_last == 0u) return;

  // ---- phase 2: the reducer
  float *red = reinterpret_cast<float *>(lds + 1);
  float mn = INFINITY;
  for (int i = tid; i < S; i += AMPPI_THREADS) mn = fminf(mn, a.costs[i]);
  const float beta = block_reduce<RED_MIN>(mn, red);
  const float nil = (float)(-1.0 / (double)a.lambda);  // (-1 / lambda_) is a Python float, amppi.py:251
  double z = 0.0;
  for (int i = tid; i < S; i += AMPPI_THREADS) z += (double)expf(nil * (a.costs[i] - beta));
  z = wave_sum_d(z);
  wg_sync();
  if ((tid & 63) == 0) lds[9 + (tid >> 6)] = z;
  wg_sync();
  const float eta = (float)log(((lds[9] + lds[10]) + lds[11]) + lds[12]);  // logsumexp: the largest entry of log_costs is 0
  for (int i = tid; i < S; i += AMPPI_THREADS) a.omega[i] = nil * (a.costs[i] - beta) - eta;
  // a_seq += tensordot(exp(omega), eps): column j by lane (q, j), q strides the samples; the q partials are added in order
  const int nq = AMPPI_THREADS / D, q = tid / D, j = tid - q * D;
  double acc = 0.0;
  if (q < nq) {
    const float aj = a.a_seq[j];
    for (int i = q; i < S; i += nq) {
      const float w = expf((nil * (a.costs[i] - beta)) - eta);
      acc += (double)w * (double)(a.acts[(size_t)i * D + j] - aj);
    }
  }
  lds[16 + tid] = acc;
  wg_sync();
  if (tid < D) {
    double sum = 0.0;
    for (int k = 0; k < nq; ++k) sum += lds[16 + k * D + tid];
    const int d = da == 2 ? (tid & 1) : 0;
    a.a_seq[tid] = clampf(a.a_seq[tid] + (float)sum, a.min_a[d], a.max_a[d]);
  }
  if (tid == 0 && a.philox) a.ctr[1] += 1u;

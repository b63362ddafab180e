// forward.h -- the two phases of the solve kernel's iteration after the backward sweep (kernels.h
// "forward sweep" and "bound-dual step, fraction to boundary"): forward_sweep, the step dw and the
// multiplier step from the gains and the value function; bound_step, a lane's bound-dual steps and its
// fraction-to-boundary limits (the main step and the second-order correction both call it); and
// step_lengths, the main step's group reduction to amax, az, the directional derivative gd and the
// tiny-step flag.  Operands are arguments (no captures of the kernel's state), so
// tests/hip/forward_check.hip calls the very functions the kernel runs.  Included by kernels.h after
// backward.h.
#pragma once

namespace mpcx {

// ---- forward sweep: dw (lane k-1 -> k).  On node lane k, with the stage Jacobians Af, Bf (inside
// the model's masks), the gains Kk, the value function Pk, the multiplier lam and the right-hand
// sides cc (defect), kf (feed-forward), pv (p_k), c0v (x0 - X_0, used on lane 0):
//   dx_0 = c0v;  dx_1 = cc_0 + B_0 kf_0 whatever A_0 and K_0 hold (interval 0 integrates from x0:
//   A_0 = 0; the kernel zeroes K_0);  dx_{k+1} = (A_k + B_k K_k) dx_k + cc_k + B_k kf_k;
//   dzo = (dx_k, du_k = kf_k + K_k dx_k; du_N = 0);  dlo = P_k dx_k + pv_k - lam_k;
// zeros on the lanes without a node (!hasX).  Every lane of the block calls it (DPP partners, and
// for G > 64 barriers: XWave<G>::W exchanges per call, the slot carries on in xw).
template <class Model, int G>
__device__ __forceinline__ void forward_sweep(int k, int N, bool hasX, const double* Af, const double* Bf,
                                              const double* Kk, const double* Pk, const double* lam, const double* cc,
                                              const double* kf, const double* pv, const double* c0v, XWave<G>& xw,
                                              double* dzo, double* dlo) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU;
  const int lane = threadIdx.x & 63;
  // closed-loop map of the step, node-parallel (off the sequential chain):
  // dx_{k+1} = (A + B K) dx_k + (c + B k_f);  du_k = k_f + K dx_k afterwards
  double Acl[NX * NX], ccl[NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) {
    double acc = cc[r];
#pragma unroll
    for (int l = 0; l < NU; ++l)
      if (Model::BMASK & (1ull << (r * NU + l))) acc = fma(Bf[r * NU + l], kf[l], acc);
    ccl[r] = acc;
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      double e = (Model::AMASK & (1ull << (r * NX + m))) ? Af[r * NX + m] : 0.0;
#pragma unroll
      for (int l = 0; l < NU; ++l)
        if (Model::BMASK & (1ull << (r * NU + l))) e = fma(Bf[r * NU + l], Kk[l * NX + m], e);
      Acl[r * NX + m] = e;
    }
  }
  {
    // dx_k = T_{k-1}( ... T_0(c0)) with affine T_j(x) = Acl_j x + ccl_j: an inclusive
    // parallel prefix of map compositions (log2 GW levels per wave, all lanes busy) instead
    // of N+1 dependent steps.  Lane k starts with T_{k-1} (lane 0: the constant map c0) and
    // composes with the partial map of its DPP partner at each level: Kogge-Stone inside
    // each 16-lane row, then the previous rows' totals by row broadcasts (scan_partner; the
    // ds_bpermute version of the same scan, Hillis-Steele over lane k-d: config 2 16.3 us per
    // IPM iteration against 15.8 us with the DPP partners, config 3 35.0 against 33.7 us).
    // Multi-wave groups scan every wave at once; the first lane of wave w gets
    // T_{64w-1} from wave w-1 through LDS, and the waves' partial results are chained
    // by one LDS handoff of dx per wave boundary.
    constexpr int NM = NX * NX + NX;
    constexpr int GW = G < 64 ? G : 64;  // lanes scanned per wave
    const int wv = G > 64 ? (int)(threadIdx.x >> 6) : 0;
    double Am[NX * NX], cm[NX];
    {
      double own[NM], prv[NM];
#pragma unroll
      for (int i = 0; i < NX * NX; ++i) own[i] = Acl[i];
#pragma unroll
      for (int i = 0; i < NX; ++i) own[NX * NX + i] = ccl[i];
#pragma unroll
      for (int i = 0; i < NM; ++i) prv[i] = from_prev(own[i]);
      if constexpr (G > 64) {  // lane 0 of wave w > 0: T_{64w-1} lives on lane 63 of wave w-1
        double* b = xw.cur();
        if (lane == 63 && wv < XWave<G>::W - 1)
#pragma unroll
          for (int i = 0; i < NM; ++i) b[wv * kXchStride + i] = own[i];
        xw.sync();
        if (lane == 0 && wv > 0)
#pragma unroll
          for (int i = 0; i < NM; ++i) prv[i] = xw.prev()[(wv - 1) * kXchStride + i];
      }
      // lane 1 takes only T_0's constant part: dx_1 = B_0 du_0 + c_1 does not depend on dx_0
      // (interval 0 integrates from x0, A_0 = 0)
#pragma unroll
      for (int i = 0; i < NX * NX; ++i) Am[i] = (k <= 1) ? 0.0 : prv[i];
#pragma unroll
      for (int i = 0; i < NX; ++i) cm[i] = (k == 0) ? c0v[i] : prv[NX * NX + i];
    }
    const int kw = k & (GW - 1);  // position inside the wave
    // one level: compose with the partial map of the DPP partner (collectives.h scan_partner)
    auto level = [&](auto dc) __attribute__((always_inline)) {
      constexpr int d = decltype(dc)::value;
      if constexpr (d < GW) {
        double Ao[NX * NX], co[NX];
#pragma unroll
        for (int i = 0; i < NX * NX; ++i) Ao[i] = scan_partner<d>(Am[i]);
#pragma unroll
        for (int i = 0; i < NX; ++i) co[i] = scan_partner<d>(cm[i]);
        if (scan_takes<d>(kw)) {  // compose: (Am, cm) o (Ao, co)
          double An[NX * NX], cn[NX];
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            double acc = cm[r];
#pragma unroll
            for (int m = 0; m < NX; ++m) acc = fma(Am[r * NX + m], co[m], acc);
            cn[r] = acc;
#pragma unroll
            for (int c = 0; c < NX; ++c) {
              double e = Am[r * NX] * Ao[c];
#pragma unroll
              for (int m = 1; m < NX; ++m) e = fma(Am[r * NX + m], Ao[m * NX + c], e);
              An[r * NX + c] = e;
            }
          }
#pragma unroll
          for (int i = 0; i < NX * NX; ++i) Am[i] = An[i];
#pragma unroll
          for (int i = 0; i < NX; ++i) cm[i] = cn[i];
        }
      }
    };
    level(std::integral_constant<int, 1>{});
    level(std::integral_constant<int, 2>{});
    level(std::integral_constant<int, 4>{});
    level(std::integral_constant<int, 8>{});
    level(std::integral_constant<int, 16>{});
    level(std::integral_constant<int, 32>{});
    if constexpr (G > 64) {
      // wave w's lanes hold maps dx_{64w-1} -> dx_k; chain the waves in order
      for (int ph = 1; ph < XWave<G>::W; ++ph) {
        double* b = xw.cur();
        if (wv == ph - 1 && lane == 63)
#pragma unroll
          for (int i = 0; i < NX; ++i) b[i] = cm[i];
        xw.sync();
        if (wv == ph) {
          const double* in = xw.prev();
          double cn[NX];
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            double acc = cm[r];
#pragma unroll
            for (int m = 0; m < NX; ++m) acc = fma(Am[r * NX + m], in[m], acc);
            cn[r] = acc;
          }
#pragma unroll
          for (int i = 0; i < NX; ++i) cm[i] = cn[i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) dzo[i] = cm[i];
  }
  // du_k = k_f + K dx_k on all lanes at once (the last node has no control)
#pragma unroll
  for (int l = 0; l < NU; ++l) {
    double acc = kf[l];
#pragma unroll
    for (int m = 0; m < NX; ++m) acc = fma(Kk[l * NX + m], dzo[m], acc);
    dzo[NX + l] = (k < N) ? acc : 0.0;
  }
  // lambda+ = P_k dx_k + p_k (node-parallel, after the sequential sweep)
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    double acc = pv[i];
#pragma unroll
    for (int m = 0; m < NX; ++m) acc = fma(Pk[symix(i, m, NX)], dzo[m], acc);
    dlo[i] = acc - lam[i];
  }
  if (!hasX) {
#pragma unroll
    for (int i = 0; i < NZ; ++i) dzo[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) dlo[i] = 0.0;
  }
}

// ---- bound-dual step and fraction to the boundary, this lane's part.  For each bounded component
// (hL / hU) with slack s = z - lb or ub - z:  dzL = mu / s - zL - zL dz / s,  dzU = mu / s - zU +
// zU dz / s (zero where there is no bound), and the largest steps that keep the slacks and the bound
// multipliers at (1 - tau) of their values:  amax_l = min(1, tau s / |dz| over the components moving
// towards their bound),  az_l = min(1, tau zL / -dzL, tau zU / -dzU over the decreasing multipliers).
// rcp64 of a zero or NaN step is NaN, but such a value is only used under a comparison that is false
// for both (collectives.h rcp64).
template <int NZ, class BL = const double*, class BU = const double*>
__device__ __forceinline__ void bound_step(const double* z, const double* dz, const BL& lb, const BU& ub, const bool* hL,
                                           const bool* hU, const double* zL, const double* zU, double mu, double tau,
                                           double* dzL, double* dzU, double& amax_l, double& az_l) {
  amax_l = 1.0;
  az_l = 1.0;
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    dzL[i] = dzU[i] = 0.0;
    const double rdz = rcp64(dz[i]);
    if (hL[i]) {
      const double s = z[i] - lb[i], rs = rcp64(s);
      dzL[i] = fma(mu, rs, -zL[i]) - zL[i] * rs * dz[i];
      if (dz[i] < 0) amax_l = fmin(amax_l, -tau * s * rdz);
      if (dzL[i] < 0) az_l = fmin(az_l, -tau * zL[i] * rcp64(dzL[i]));
    }
    if (hU[i]) {
      const double s = ub[i] - z[i], rs = rcp64(s);
      dzU[i] = fma(mu, rs, -zU[i]) + zU[i] * rs * dz[i];
      if (dz[i] > 0) amax_l = fmin(amax_l, tau * s * rdz);
      if (dzU[i] < 0) az_l = fmin(az_l, -tau * zU[i] * rcp64(dzU[i]));
    }
  }
}

// ---- the main step's lengths over the group: amax, az (min of the lanes' limits), the barrier
// objective's directional derivative gd = sum gp_i dz_i and IPOPT's tiny-step test
// max |dz_i| / (1 + |z_i|) < 10 eps, both over the entries the lanes own (x of a node lane, u of a
// lane with a control).  The test is taken as the sign of |dz_i| - 10 eps (1 + |z_i|) (one fma, no
// reciprocal); a lane's entries it does not own count neither for gd nor for the test.  One
// exchange: a 4-value reduction for G > 64, a 3-value one and a ballot otherwise.
template <int G, int R, int NX, int NU>
__device__ __forceinline__ void step_lengths(bool hasX, bool hasU, const double* z, const double* dz, const double* gp,
                                             double amax_l, double az_l, XWave<G>& xw, double& amax, double& az,
                                             double& gd, bool& tinystep) {
  double tiny_l = -1.0, gd_l = 0.0;
#pragma unroll
  for (int i = 0; i < NX + NU; ++i) {
    const bool own = (i < NX) ? hasX : hasU;
    tiny_l = qmax(tiny_l, own ? fma(-10.0 * kEps, 1.0 + fabs(z[i]), fabs(dz[i])) : -1.0);
    if (own) gd_l += gp[i] * dz[i];
  }
  // amax, az (min), gd (sum) and the tiny-step test (max over the group < 0) in one exchange
  double fr[4] = {amax_l, az_l, gd_l, tiny_l < 0.0 ? 1.0 : 0.0};
  if constexpr (G > 64) {
    greduce_n<G, 2, 2, 0, 3>(fr, xw);
  } else {
    greduce_n<G, 2, 2, 0>(fr, xw);
    fr[3] = gall<G, G * R>(tiny_l < 0.0, xw) ? 1.0 : 0.0;
  }
  amax = fr[0];
  az = fr[1];
  gd = fr[2];
  tinystep = fr[3] > 0.5;
}

}  // namespace mpcx

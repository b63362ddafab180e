// suffix_check.hip -- test harness for the reused decoupled suffix of the linear models (backward.h
// dec_suffix_setup, dec_suffix_split, suffix_scan) in multi-wave groups: LinearModel<5, 1>, one
// instance per block of G = 128 or 256 lanes.  Three passes over the same operands, each through the
// solve kernel's own sweeps: (1) the fresh factorisation (backward_chain_waves, every step a full
// one), whose P_k become the stored Pk; (2) the reused suffix as a chain (dec_suffix_setup,
// dec_suffix_split, backward_chain_waves); (3) the reused suffix as the radix-4 scan (suffix_scan
// before the chain).  Per node and pass it writes P_k, p_k, the factors' g0 and the lane's inertia
// verdict; per instance whether the scan ran.  A second entry point runs the passes twice in one
// launch, on two schedules, with the scan's cached matrix powers carried from the first to the second.
// Built into tests/hip/libsuffix_check.so (tests/hip/Makefile); used by tests/test_gpu_scan.py only.
#include "kernels.h"

namespace mpcx {

using SufModel = LinearModel<5, 1>;
// per node, in: Hs 21 (packed upper, z = (x, u)), Sigma 6, gp 6, B 5, c 5; A comes from the instance's
// stage tables (n_tab tables of 25) through the schedule (one table index per node)
constexpr int kSufIn = 21 + 6 + 6 + 5 + 5;
// per node and pass, out: P 15, p 5, g0, okl
constexpr int kSufOut = 15 + 5 + 2;

// The three passes of this block's instance on schedule `tab` (G entries, clamped to the n_tab tables);
// out: 3 * G node records (pass-major) or null, ran: whether pass 3's scan ran, or null
template <int G>
__device__ __forceinline__ void suffix_passes(int N, int kb, bool shared_tables, const double* in, const double* Atab,
                                              int n_tab, const int* tab, double* dscan, double& pow_tab, XWave<G>& xw,
                                              double* out, int* ran) {
  using M = SufModel;
  constexpr int NX = 5, NZ = 6, NH = 21, NP = 15;
  const int k = (int)threadIdx.x;
  double Hd[NH], sgv[NZ], gp[NZ], A[NX * NX], Bm[NX], c[NX];
  const double* r = in + k * kSufIn;
  for (int i = 0; i < NH; ++i) Hd[i] = *r++;
  for (int i = 0; i < NZ; ++i) sgv[i] = *r++;
  for (int i = 0; i < NZ; ++i) gp[i] = *r++;
  for (int i = 0; i < NX; ++i) Bm[i] = *r++;
  for (int i = 0; i < NX; ++i) c[i] = *r++;
  const double* Amine = Atab + min(max(tab[k], 0), n_tab - 1) * NX * NX;  // this lane's stage table
  for (int i = 0; i < NX * NX; ++i) A[i] = Amine[i];
  const double delta = 0.0;  // (a factorisation reuses the suffix only at delta = 0)
#pragma unroll
  for (int i = 0; i < NZ; ++i) Hd[symix(i, i, NZ)] += sgv[i] + delta;
  auto put = [&](int pass, const double* P, const double* p, const Fac<5, 1>& f, bool okl) {
    if (out == nullptr || k > N) return;
    double* o = out + ((long)pass * G + k) * kSufOut;
    for (int i = 0; i < NP; ++i) o[i] = P[i];
    for (int i = 0; i < NX; ++i) o[NP + i] = p[i];
    o[NP + NX] = f.g0;
    o[NP + NX + 1] = okl ? 1.0 : 0.0;
  };
  // ---- pass 1: the fresh factorisation
  double Pk[NP];
  {
    double P[NP], p[NX];
    Fac<5, 1> fac = {};
    bool okl = true;
    terminal_value<NX>(k, N, sgv, delta, gp, P, p);
    DecSuffix<M> ds;
    ds.reuse = false;
    ds.kb = kb;
    ds.jc = N;
    backward_chain_waves<M, G>(k, N, true, ds, false, Hd, gp, A, Bm, c, xw, P, p, fac, okl);
    put(0, P, p, fac, okl);
    for (int i = 0; i < NP; ++i) Pk[i] = P[i];
  }
  // ---- passes 2 and 3: the reused suffix, as a chain and with the scan
  for (int pass = 1; pass <= 2; ++pass) {
    double P[NP], p[NX];
    Fac<5, 1> fac = {};
    bool okl = true;
    terminal_value<NX>(k, N, sgv, delta, gp, P, p);
    DecSuffix<M> ds;
    ds.reuse = true;
    ds.kb = kb;
    ds.jc = N;
    dec_suffix_setup<M, G>(k, N, Hd, c, Pk, xw, ds, P, fac);
    ds.jc = dec_suffix_split<G>(true, kb, N);
    bool sscan = false;
    if (pass == 2) {
      sscan = suffix_scan<M, G>(k, N, true, ds, shared_tables, Atab, Amine, gp, Amine, dscan, pow_tab, xw, p, fac, okl);
      if (ran != nullptr && k == 0) *ran = sscan ? 1 : 0;
    }
    backward_chain_waves<M, G>(k, N, true, ds, sscan, Hd, gp, A, Bm, c, xw, P, p, fac, okl);
    put(pass, P, p, fac, okl);
  }
}

// one instance per block; in: G node records per instance, Atab: n_tab tables per instance, tab: G
// table indices per instance; out: 3 * G node records per instance, ran: one int per instance
template <int G>
__global__ __launch_bounds__(G) void suffix_check_kernel(int N, int kb, int n_tab, int shared_tables, const double* in,
                                                         const double* Atab, const int* tab, double* out, int* ran) {
  __shared__ double xch[2 * XWave<G>::W * kXchStride];
  __shared__ double dscan[2 * 5 * G + 15 * 5 * 5];
  XWave<G> xw{xch, 0};
  double pow_tab = -1.0;
  const long b = blockIdx.x;
  suffix_passes<G>(N, kb, shared_tables != 0, in + b * G * kSufIn, Atab + b * n_tab * 25, n_tab, tab + b * G, dscan,
                   pow_tab, xw, out + b * 3 * G * kSufOut, ran + b);
}

// the passes on schedule tab0, then -- the same launch, the powers cached for tab0's suffix table still
// in LDS -- on schedule tab1, whose results are the ones written
template <int G>
__global__ __launch_bounds__(G) void suffix_twice_kernel(int N, int kb, int n_tab, const double* in, const double* Atab,
                                                         const int* tab0, const int* tab1, double* out, int* ran) {
  __shared__ double xch[2 * XWave<G>::W * kXchStride];
  __shared__ double dscan[2 * 5 * G + 15 * 5 * 5];
  XWave<G> xw{xch, 0};
  double pow_tab = -1.0;
  const long b = blockIdx.x;
  suffix_passes<G>(N, kb, true, in + b * G * kSufIn, Atab + b * n_tab * 25, n_tab, tab0 + b * G, dscan, pow_tab, xw, nullptr,
                   nullptr);
  suffix_passes<G>(N, kb, true, in + b * G * kSufIn, Atab + b * n_tab * 25, n_tab, tab1 + b * G, dscan, pow_tab, xw,
                   out + b * 3 * G * kSufOut, ran + b);
}

}  // namespace mpcx

// G = 128 or 256, 1 <= N < G, 0 <= kb <= N, B blocks.  in: B * G * 43 doubles, Atab: B * n_tab * 25
// doubles, tab: B * G ints (clamped to [0, n_tab)), out: B * 3 * G * 22 doubles, ran: B ints (device
// pointers).  1: bad shape, 2: no such G, 3: the launch failed
extern "C" int suffix_check(int G, int N, int kb, int B, int n_tab, int shared_tables, const double* in,
                            const double* Atab, const int* tab, double* out, int* ran) {
  if (B <= 0 || N < 1 || N >= G || kb < 0 || kb > N || n_tab < 1) return 1;
  if (G == 128)
    hipLaunchKernelGGL(mpcx::suffix_check_kernel<128>, dim3(B), dim3(128), 0, 0, N, kb, n_tab, shared_tables, in, Atab, tab,
                       out, ran);
  else if (G == 256)
    hipLaunchKernelGGL(mpcx::suffix_check_kernel<256>, dim3(B), dim3(256), 0, 0, N, kb, n_tab, shared_tables, in, Atab, tab,
                       out, ran);
  else
    return 2;
  return hipDeviceSynchronize() == hipSuccess ? 0 : 3;
}

// as suffix_check with shared tables, run on tab0 and then, in the same launch, on tab1
extern "C" int suffix_check_twice(int G, int N, int kb, int B, int n_tab, const double* in, const double* Atab,
                                  const int* tab0, const int* tab1, double* out, int* ran) {
  if (B <= 0 || N < 1 || N >= G || kb < 0 || kb > N || n_tab < 1) return 1;
  if (G == 128)
    hipLaunchKernelGGL(mpcx::suffix_twice_kernel<128>, dim3(B), dim3(128), 0, 0, N, kb, n_tab, in, Atab, tab0, tab1, out,
                       ran);
  else if (G == 256)
    hipLaunchKernelGGL(mpcx::suffix_twice_kernel<256>, dim3(B), dim3(256), 0, 0, N, kb, n_tab, in, Atab, tab0, tab1, out,
                       ran);
  else
    return 2;
  return hipDeviceSynchronize() == hipSuccess ? 0 : 3;
}

// scan_check.hip -- test harness for the log-depth Riccati scan (backward.h backward_scan, pscan.h
// relem_stage / relem_combine_lds) and for the sequential chains it falls back to (backward_chain in
// single-wave groups, several instances per wave included; backward_chain_waves in multi-wave groups).
// The kernel forms the stage operands as the solve kernel does (Hd = stage Hessian + Sigma + delta),
// calls the solve kernel's own sweeps -- the scan first, then, on the same operands, the path taken
// when the scan reports "take the sequential recursion" -- and writes per node the value function
// (P_k, p_k), every field of the step's factors, the gains recovered from them and the lane's inertia
// verdict, once for each path, and per instance the scan's fallback flag.  Built into
// tests/hip/libscan_check.so (tests/hip/Makefile); used by tests/test_gpu_scan.py only, which compares
// with a long-double recursion in numpy.
#include "kernels.h"

namespace mpcx {

// per node, in: Hs NH (packed upper, z = (x, u); without Sigma and delta), Sigma NZ, gp NZ, A NX^2,
// B NX NU, c NX
template <class Model>
constexpr int scan_in() {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU;
  return NZ * (NZ + 1) / 2 + 2 * NZ + NX * NX + NX * NU + NX;
}
// per node, out: P NP, p NX, fac (r0, r1, t, h0 NX, h1 NX, g0, g1), K NU NX, kf NU, okl, fac_ok
template <class Model>
constexpr int scan_out() {
  return Model::NX * (Model::NX + 1) / 2 + Model::NX + 5 + 2 * Model::NX + Model::NU * Model::NX + Model::NU + 2;
}

template <int NX, int NU>
__device__ void put_record(double* o, const double* P, const double* p, const Fac<NX, NU>& f, bool okl) {
  constexpr int NP = NX * (NX + 1) / 2;
  double K[NU * NX], kf[NU];
  riccati_gains<NX, NU>(f, K, kf);
  for (int i = 0; i < NP; ++i) *o++ = P[i];
  for (int i = 0; i < NX; ++i) *o++ = p[i];
  *o++ = f.r0;
  *o++ = f.r1;
  *o++ = f.t;
  for (int i = 0; i < NX; ++i) *o++ = f.h0[i];
  for (int i = 0; i < NX; ++i) *o++ = f.h1[i];
  *o++ = f.g0;
  *o++ = f.g1;
  for (int i = 0; i < NU * NX; ++i) *o++ = K[i];
  for (int i = 0; i < NU; ++i) *o++ = kf[i];
  *o++ = okl ? 1.0 : 0.0;
  *o++ = fac_ok<NX, NU>(f) ? 1.0 : 0.0;
}

// in: B * G node records; out_scan, out_seq: B * G node records (nodes 0..N written); flag: B ints.
// Lanes of instances at or beyond B and lanes beyond N take part in every call with hasU = hasX =
// false, as in the solve kernel: no lane leaves before the barriers.
template <class Model, int G>
__global__ __launch_bounds__(G > 64 ? G : 64) void scan_check_kernel(int N, int B, double delta, const double* in,
                                                                    double* out_scan, double* out_seq, int* flag) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NH = NZ * (NZ + 1) / 2, NP = NX * (NX + 1) / 2;
  constexpr int kSBS = G > 64 ? G : 64;
  constexpr int kIn = scan_in<Model>(), kOut = scan_out<Model>();
  __shared__ double sbuf[RElem<NX>::NE * kSBS];
  __shared__ double xch[2 * XWave<G>::W * kXchStride];
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));
  const int inst = (int)(gid / G);
  const bool valid = inst < B;
  const bool hasX = valid && k <= N, hasU = valid && k < N;
  double Hd[NH] = {}, sgv[NZ] = {}, gp[NZ] = {}, A[NX * NX] = {}, Bm[NX * NU] = {}, c[NX] = {};
  if (hasX) {
    const double* r = in + ((long)inst * G + k) * kIn;
    for (int i = 0; i < NH; ++i) Hd[i] = *r++;
    for (int i = 0; i < NZ; ++i) sgv[i] = *r++;
    for (int i = 0; i < NZ; ++i) gp[i] = *r++;
    for (int i = 0; i < NX * NX; ++i) A[i] = *r++;
    for (int i = 0; i < NX * NU; ++i) Bm[i] = *r++;
    for (int i = 0; i < NX; ++i) c[i] = *r++;
  }
#pragma unroll
  for (int i = 0; i < NZ; ++i) Hd[symix(i, i, NZ)] += sgv[i] + delta;  // the solve kernel's order
  XWave<G> xw{xch, 0};
  // ---- the scan and its node-parallel step
  double P[NP], p[NX];
  Fac<NX, NU> fac = {};
  bool okl = true;
  const bool seq = backward_scan<Model, G, 1>(k, N, hasU, hasX, Hd, sgv, delta, gp, A, Bm, c, sbuf, xw, P, p, fac, okl);
  if (hasX) put_record<NX, NU>(out_scan + ((long)inst * G + k) * kOut, P, p, fac, okl);
  if (valid && k == 0) flag[inst] = seq ? 1 : 0;
  // ---- the path taken when the flag is set, on the same operands
  double P2[NP], p2[NX];
  Fac<NX, NU> fac2 = {};
  bool okl2 = true;
  terminal_value<NX>(k, N, sgv, delta, gp, P2, p2);
  DecSuffix<Model> ds;  // no decoupled suffix: every step is a full one
  ds.kb = N + 1;
  ds.jc = N;
  if constexpr (G <= 64)
    backward_chain<Model, G>(k, N, hasU, valid, ds, Hd, delta, gp, A, Bm, c, nullptr, 0, gid, P2, p2, fac2, okl2);
  else
    backward_chain_waves<Model, G>(k, N, valid, ds, false, Hd, gp, A, Bm, c, xw, P2, p2, fac2, okl2);
  if (hasX) put_record<NX, NU>(out_seq + ((long)inst * G + k) * kOut, P2, p2, fac2, okl2);
}

template <class Model, int G>
int launch_scan_check(int N, int B, double delta, const double* in, double* out_scan, double* out_seq, int* flag) {
  constexpr int kBlock = G > 64 ? G : 64;
  const int blocks = (int)(((long)B * G + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((scan_check_kernel<Model, G>), dim3(blocks), dim3(kBlock), 0, 0, N, B, delta, in, out_scan, out_seq,
                     flag);
  return hipDeviceSynchronize() == hipSuccess ? 0 : 3;
}

}  // namespace mpcx

// the record sizes of a model (doubles per node, in and out); 2: no such model
extern "C" int scan_check_sizes(int model, int* n_in, int* n_out) {
  using namespace mpcx;
  switch (model) {
    case 0: *n_in = scan_in<UnicycleScanModel>(), *n_out = scan_out<UnicycleScanModel>(); return 0;
    case 1: *n_in = scan_in<LinearModel<4, 1>>(), *n_out = scan_out<LinearModel<4, 1>>(); return 0;
    case 2: *n_in = scan_in<LinearModel<4, 2>>(), *n_out = scan_out<LinearModel<4, 2>>(); return 0;
    case 3: *n_in = scan_in<OdeModel<KinBicycle>>(), *n_out = scan_out<OdeModel<KinBicycle>>(); return 0;
  }
  return 2;
}

// model: 0 UnicycleScanModel (G = 32, 64, 128), 1 LinearModel<4, 1> (G = 16, 32, 64, 128, 256),
// 2 LinearModel<4, 2> (G = 64), 3 OdeModel<KinBicycle> (G = 64).  in: B * G * n_in doubles, out_scan,
// out_seq: B * G * n_out doubles, flag: B ints (device pointers).  1: bad shape, 2: no such
// instantiation, 3: the launch failed
extern "C" int scan_check(int model, int G, int N, int B, double delta, const double* in, double* out_scan,
                          double* out_seq, int* flag) {
  using namespace mpcx;
  if (B <= 0 || N < 1 || N >= G) return 1;
  using Lin41 = LinearModel<4, 1>;
  using Lin42 = LinearModel<4, 2>;
  using KinBike = OdeModel<KinBicycle>;
#define MPCX_SCAN_CASE(id, M, g) \
  if (model == id && G == g) return launch_scan_check<M, g>(N, B, delta, in, out_scan, out_seq, flag);
  MPCX_SCAN_CASE(0, UnicycleScanModel, 32)
  MPCX_SCAN_CASE(0, UnicycleScanModel, 64)
  MPCX_SCAN_CASE(0, UnicycleScanModel, 128)
  MPCX_SCAN_CASE(1, Lin41, 16)
  MPCX_SCAN_CASE(1, Lin41, 32)
  MPCX_SCAN_CASE(1, Lin41, 64)
  MPCX_SCAN_CASE(1, Lin41, 128)
  MPCX_SCAN_CASE(1, Lin41, 256)
  MPCX_SCAN_CASE(2, Lin42, 64)
  MPCX_SCAN_CASE(3, KinBike, 64)
#undef MPCX_SCAN_CASE
  return 2;
}

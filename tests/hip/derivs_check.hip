// derivs_check.hip -- test harness for the ODE models' stage derivatives (mpc-verde_amd/csrc/ode.h):
// one thread per point evaluates OdeModel<Dyn>::derivs (the solve kernel's dispatch), derivs_passes
// or value at (z, lam, stage row, fs), with the per-lane LDS value cache laid out as the solve
// kernel lays it out, or without it.  tests/test_gpu_stage_derivs.py compares the output with the
// extended-precision reference tests/helpers/stage_derivs_ref.py.  Built into
// tests/hip/libderivs_check.so; not part of libmpcx.
#include "models.h"
#include "ode.h"
#include "riccati.h"

namespace mpcx {

// WHICH: 0 Model::derivs, 1 Model::derivs_passes, 2 Model::value (xf, q only)
// out per point: xf NX, q 1, A NX^2, B NX NU, g NZ, H NZ (NZ + 1) / 2 (flop_probe.hip's order)
template <class Model, int WHICH>
__global__ void derivs_check_kernel(int n, ModelArgs ma, int k, int use_cache, double fs, const double* Z, const double* L,
                                    const double* P, int pstride, double* out) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NH = NZ * (NZ + 1) / 2;
  constexpr int NO = NX + 1 + NX * NX + NX * NU + NZ + NH;
  extern __shared__ double tcbuf[];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (use_cache) {
    ma.tc = tcbuf + threadIdx.x;
    ma.tc_stride = blockDim.x;
  }
  typename Model::Ctx c;
  Model::load_ctx(ma, i, P + (size_t)i * pstride, k, true, c);
  double z[NZ], ln[NX];
  for (int j = 0; j < NZ; ++j) z[j] = Z[(size_t)i * NZ + j];
  for (int j = 0; j < NX; ++j) ln[j] = L[(size_t)i * NX + j];
  double xf[NX], q;
  double* o = out + (size_t)i * NO;
  int t = 0;
  if constexpr (WHICH == 2) {
    Model::value(ma, c, z, xf, q);
    for (int j = 0; j < NX; ++j) o[t++] = xf[j];
    o[t++] = q;
  } else {
    double A[NX * NX], Bm[NX * NU], g[NZ], H[NH];
    if constexpr (WHICH == 1)
      Model::derivs_passes(ma, c, z, ln, fs, xf, q, A, Bm, g, H);
    else
      Model::derivs(ma, c, z, ln, fs, xf, q, A, Bm, g, H);
    for (int j = 0; j < NX; ++j) o[t++] = xf[j];
    o[t++] = q;
    for (int j = 0; j < NX * NX; ++j) o[t++] = A[j];
    for (int j = 0; j < NX * NU; ++j) o[t++] = Bm[j];
    for (int j = 0; j < NZ; ++j) o[t++] = g[j];
    for (int j = 0; j < NH; ++j) o[t++] = H[j];
  }
}

template <class Model, int WHICH>
int launch_one(int n, const ModelArgs& ma, int k, int use_cache, double fs, const double* Z, const double* L,
               const double* P, int pstride, double* out) {
  const size_t lds = (size_t)Model::kTrigSlots * 64 * sizeof(double);
  hipLaunchKernelGGL((derivs_check_kernel<Model, WHICH>), dim3(n / 64), dim3(64), lds, 0, n, ma, k, use_cache, fs, Z, L, P,
                     pstride, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return -1000 - (int)e;
  const hipError_t s = hipDeviceSynchronize();
  return s == hipSuccess ? 0 : -2000 - (int)s;
}

template <class Model>
int launch_derivs(int which, int n, const ModelArgs& ma, int k, int use_cache, double fs, const double* Z, const double* L,
                  const double* P, int pstride, double* out) {
  // every row load_ctx reads lies inside this point's P row
  constexpr int NX = Model::NX, NZ = Model::NX + Model::NU;
  if (pstride < (ma.p_layout == 0 ? 2 * NX : NX + NZ * (k + 1))) return -3;
  switch (which) {
    case 0: return launch_one<Model, 0>(n, ma, k, use_cache, fs, Z, L, P, pstride, out);
    case 1: return launch_one<Model, 1>(n, ma, k, use_cache, fs, Z, L, P, pstride, out);
    default: return launch_one<Model, 2>(n, ma, k, use_cache, fs, Z, L, P, pstride, out);
  }
}

}  // namespace mpcx

// model: 3 kinematic bicycle, 4 dynamic bicycle, 5 cart-pole, 6 path-frame bicycle (7, its id in
// include/mpcx.h, is accepted too).  Z: n x NZ, L: n x NX, P: n x pstride (x0, then the target
// [p_layout 0] or the stage rows 0..k [p_layout 1]), out: n x NO, all device pointers; n a multiple
// of 64 (one unit per lane).  which: 0 derivs, 1 derivs_passes, 2 value.  use_cache 0: no LDS value
// cache (ModelArgs::tc == nullptr).  Returns 0 on success, -3 for a bad argument, -4 for an
// unknown model, -1000 - e / -2000 - e for a launch / synchronise error e.
extern "C" int derivs_check(int model, int n, double T, int M, int cost, const double* Q, const double* R,
                            const double* par, const double* Z, const double* L, const double* P, int pstride,
                            double* out, double fs, int p_layout, int k, int use_cache, int which) {
  using namespace mpcx;
  if (n <= 0 || n % 64 || M < 1 || k < 0 || which < 0 || which > 2 || (p_layout != 0 && p_layout != 1)) return -3;
  (void)cost;  // the ODE models have the node cost only
  ModelArgs ma{};
  ma.p_layout = p_layout;
  ma.N = k + 1;
  ma.op.M = M;
  ma.op.h = T / M;
  for (int j = 0; j < 8; ++j) {
    ma.op.Q[j] = Q[j];
    ma.op.R[j] = R[j];
    ma.op.par[j] = par[j];
  }
  switch (model) {
    case 3: return launch_derivs<OdeModel<KinBicycle>>(which, n, ma, k, use_cache, fs, Z, L, P, pstride, out);
    case 4: return launch_derivs<OdeModel<DynBicycle>>(which, n, ma, k, use_cache, fs, Z, L, P, pstride, out);
    case 5: return launch_derivs<OdeModel<CartPole>>(which, n, ma, k, use_cache, fs, Z, L, P, pstride, out);
    case 6:
    case 7: return launch_derivs<OdeModel<PathBicycle>>(which, n, ma, k, use_cache, fs, Z, L, P, pstride, out);
    default: return -4;
  }
}

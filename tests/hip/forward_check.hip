// forward_check.hip -- test harness for the two phases of the solve kernel's iteration after the
// backward sweep (forward.h): forward_sweep, bound_step and step_lengths, called as the kernel calls
// them.  One launch makes the main step's calls -- the sweep, the lane's bound-dual step, the group's
// step lengths -- and then the second-order correction's: the sweep again with other right-hand
// sides and the same gains and value function (the LDS exchange slot carries over: the step lengths'
// exchange between the two leaves it flipped for multi-wave groups), the bound-dual step along the
// correction and the kernel's two group minima.  A node's record may replace the first sweep's dz
// before the bound-dual step, so a test can place a step component exactly.  Built into
// tests/hip/libforward_check.so (tests/hip/Makefile); used by tests/test_gpu_forward.py only, which
// compares with a long-double recursion in numpy (tests/helpers/forward_ref.py).
#include <cstdio>

#include "kernels.h"

namespace mpcx {

// per node, in: A NX^2, B NX NU, K NU NX, P NP (packed upper), lam NX, two right-hand sides
// (cc NX, kf NU, pv NX, c0v NX) -- the main step's, the correction's --, then z, lb, ub, hL, hU
// (0 / 1), zL, zU, gp, dz_override NZ each and one flag: use dz_override
template <class Model>
constexpr int forward_in() {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU;
  return NX * NX + NX * NU + NU * NX + NX * (NX + 1) / 2 + NX + 2 * (3 * NX + NU) + 9 * NZ + 1;
}
// per node, out: dz NZ, dlam NX (main step), dz NZ, dlam NX (correction), dzL, dzU NZ (main step),
// dzL, dzU NZ (correction)
template <class Model>
constexpr int forward_out() {
  return 2 * (Model::NX + Model::NU + Model::NX) + 4 * (Model::NX + Model::NU);
}
// per instance, out: amax, az, gd, tiny (main step); amax, az (correction)
constexpr int kForwardInst = 6;

// in: B * G node records, every lane of an instance below B reads its own (the lanes beyond N too:
// what they hold must not matter); out: B * G node records; oinst: B * kForwardInst.  Lanes of
// instances at or beyond B and lanes beyond N take part in every call with hasX = hasU = false, as
// in the solve kernel: no lane leaves before the barriers.
template <class Model, int G>
__global__ __launch_bounds__(G > 64 ? G : 64) void forward_check_kernel(int N, int B, double mu, double tau,
                                                                       const double* in, double* out, double* oinst) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NP = NX * (NX + 1) / 2;
  constexpr int kIn = forward_in<Model>(), kOut = forward_out<Model>();
  __shared__ double xch[2 * XWave<G>::W * kXchStride];
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));
  const int inst = (int)(gid / G);
  const bool valid = inst < B;
  const bool hasX = valid && k <= N, hasU = valid && k < N;
  double A[NX * NX] = {}, Bm[NX * NU] = {}, Kk[NU * NX] = {}, Pk[NP] = {}, lam[NX] = {};
  double cc[2][NX] = {}, kf[2][NU] = {}, pv[2][NX] = {}, c0v[2][NX] = {};
  double z[NZ] = {}, lb[NZ] = {}, ub[NZ] = {}, zL[NZ] = {}, zU[NZ] = {}, gp[NZ] = {}, dzov[NZ] = {};
  bool hL[NZ] = {}, hU[NZ] = {}, use_ov = false;
  if (valid) {
    const double* r = in + ((long)inst * G + k) * kIn;
    for (int i = 0; i < NX * NX; ++i) A[i] = *r++;
    for (int i = 0; i < NX * NU; ++i) Bm[i] = *r++;
    for (int i = 0; i < NU * NX; ++i) Kk[i] = *r++;
    for (int i = 0; i < NP; ++i) Pk[i] = *r++;
    for (int i = 0; i < NX; ++i) lam[i] = *r++;
    for (int c = 0; c < 2; ++c) {
      for (int i = 0; i < NX; ++i) cc[c][i] = *r++;
      for (int i = 0; i < NU; ++i) kf[c][i] = *r++;
      for (int i = 0; i < NX; ++i) pv[c][i] = *r++;
      for (int i = 0; i < NX; ++i) c0v[c][i] = *r++;
    }
    for (int i = 0; i < NZ; ++i) z[i] = *r++;
    for (int i = 0; i < NZ; ++i) lb[i] = *r++;
    for (int i = 0; i < NZ; ++i) ub[i] = *r++;
    for (int i = 0; i < NZ; ++i) hL[i] = *r++ != 0.0;
    for (int i = 0; i < NZ; ++i) hU[i] = *r++ != 0.0;
    for (int i = 0; i < NZ; ++i) zL[i] = *r++;
    for (int i = 0; i < NZ; ++i) zU[i] = *r++;
    for (int i = 0; i < NZ; ++i) gp[i] = *r++;
    for (int i = 0; i < NZ; ++i) dzov[i] = *r++;
    use_ov = *r++ != 0.0;
  }
  XWave<G> xw{xch, 0};
  // ---- the main step
  double dz[NZ], dlam[NX], dzL[NZ], dzU[NZ];
  forward_sweep<Model, G>(k, N, hasX, A, Bm, Kk, Pk, lam, cc[0], kf[0], pv[0], c0v[0], xw, dz, dlam);
  double* o = out + ((long)inst * G + k) * kOut;
  if (valid) {
    for (int i = 0; i < NZ; ++i) *o++ = dz[i];
    for (int i = 0; i < NX; ++i) *o++ = dlam[i];
  }
  if (use_ov)
    for (int i = 0; i < NZ; ++i) dz[i] = dzov[i];
  double amax_l, az_l, amax, az, gd;
  bool tinystep;
  bound_step<NZ>(z, dz, lb, ub, hL, hU, zL, zU, mu, tau, dzL, dzU, amax_l, az_l);
  step_lengths<G, 1, NX, NU>(hasX, hasU, z, dz, gp, amax_l, az_l, xw, amax, az, gd, tinystep);
  // ---- the second-order correction's calls
  double dzs[NZ], dls[NX], dzLs[NZ], dzUs[NZ], am_l, azs_l;
  forward_sweep<Model, G>(k, N, hasX, A, Bm, Kk, Pk, lam, cc[1], kf[1], pv[1], c0v[1], xw, dzs, dls);
  bound_step<NZ>(z, dzs, lb, ub, hL, hU, zL, zU, mu, tau, dzLs, dzUs, am_l, azs_l);
  const double as = gmin<G>(am_l, xw), azs = gmin<G>(azs_l, xw);
  if (valid) {
    for (int i = 0; i < NZ; ++i) *o++ = dzs[i];
    for (int i = 0; i < NX; ++i) *o++ = dls[i];
    for (int i = 0; i < NZ; ++i) *o++ = dzL[i];
    for (int i = 0; i < NZ; ++i) *o++ = dzU[i];
    for (int i = 0; i < NZ; ++i) *o++ = dzLs[i];
    for (int i = 0; i < NZ; ++i) *o++ = dzUs[i];
    if (k == 0) {
      double* q = oinst + (long)inst * kForwardInst;
      q[0] = amax, q[1] = az, q[2] = gd, q[3] = tinystep ? 1.0 : 0.0, q[4] = as, q[5] = azs;
    }
  }
}

template <class Model, int G>
int launch_forward_check(int N, int B, double mu, double tau, const double* in, double* out, double* oinst) {
  constexpr int kBlock = G > 64 ? G : 64;
  const int blocks = (int)(((long)B * G + kBlock - 1) / kBlock);
  (void)hipGetLastError();  // (an earlier call's error is not this launch's)
  hipLaunchKernelGGL((forward_check_kernel<Model, G>), dim3(blocks), dim3(kBlock), 0, 0, N, B, mu, tau, in, out, oinst);
  hipError_t e = hipGetLastError();  // a refused launch says so here, a failed kernel at the synchronisation
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) fprintf(stderr, "forward_check<G = %d>: %s\n", G, hipGetErrorString(e));
  return e == hipSuccess ? 0 : 3;
}

template <class Model>
int forward_sizes(int* dims, unsigned long long* masks) {
  dims[0] = Model::NX, dims[1] = Model::NU, dims[2] = forward_in<Model>(), dims[3] = forward_out<Model>();
  dims[4] = kForwardInst;
  masks[0] = Model::AMASK, masks[1] = Model::BMASK;
  return 0;
}

}  // namespace mpcx

// a model's dimensions: dims = (NX, NU, doubles per node in, per node out, per instance out), masks =
// (AMASK, BMASK: bit r * NX + m / r * NU + l set where the model's Jacobian entry is read); 2: no such model
extern "C" int forward_check_sizes(int model, int* dims, unsigned long long* masks) {
  using namespace mpcx;
  switch (model) {
    case 0: return forward_sizes<UnicycleModel>(dims, masks);
    case 1: return forward_sizes<LinearModel<4, 1>>(dims, masks);
    case 2: return forward_sizes<LinearModel<4, 2>>(dims, masks);
    case 3: return forward_sizes<OdeModel<PathBicycle>>(dims, masks);
    case 4: return forward_sizes<OdeModel<DynBicycle>>(dims, masks);
  }
  return 2;
}

// model: 0 UnicycleModel (G = 16, 32, 64, 128), 1 LinearModel<4, 1> (G = 16, 32, 64, 128, 256),
// 2 LinearModel<4, 2> (G = 64), 3 OdeModel<PathBicycle> (G = 64), 4 OdeModel<DynBicycle> (NX = 6, the
// widest map: 42 values per lane; G = 64).  in: B * G * n_in doubles, out: B * G * n_out doubles,
// oinst: B * 6 doubles (device pointers).  1: bad shape, 2: no such instantiation, 3: the launch failed
extern "C" int forward_check(int model, int G, int N, int B, double mu, double tau, const double* in, double* out,
                             double* oinst) {
  using namespace mpcx;
  if (B <= 0 || N < 1 || N >= G) return 1;
  using Lin41 = LinearModel<4, 1>;
  using Lin42 = LinearModel<4, 2>;
  using PathBike = OdeModel<PathBicycle>;
  using DynBike = OdeModel<DynBicycle>;
#define MPCX_FORWARD_CASE(id, M, g) \
  if (model == id && G == g) return launch_forward_check<M, g>(N, B, mu, tau, in, out, oinst);
  MPCX_FORWARD_CASE(0, UnicycleModel, 16)
  MPCX_FORWARD_CASE(0, UnicycleModel, 32)
  MPCX_FORWARD_CASE(0, UnicycleModel, 64)
  MPCX_FORWARD_CASE(0, UnicycleModel, 128)
  MPCX_FORWARD_CASE(1, Lin41, 16)
  MPCX_FORWARD_CASE(1, Lin41, 32)
  MPCX_FORWARD_CASE(1, Lin41, 64)
  MPCX_FORWARD_CASE(1, Lin41, 128)
  MPCX_FORWARD_CASE(1, Lin41, 256)
  MPCX_FORWARD_CASE(2, Lin42, 64)
  MPCX_FORWARD_CASE(3, PathBike, 64)
  MPCX_FORWARD_CASE(4, DynBike, 64)
#undef MPCX_FORWARD_CASE
  return 2;
}

/* mpcx.h -- C ABI of the MI355X-native batched multiple-shooting MPC solver.
 *
 * The drop-in boundary for the hot path of gabrielhaj/mpc-verde.  Every entry
 * point replaces one call site of the reference's CasADi boundary (paths
 * relative to the reference repository):
 *
 *   mpcx_create         ca.nlpsol('solver', 'ipopt', prob, opts)
 *                         Casadi/multiple_shooting_casadi.py:181-197
 *                         (problem = the NLP built at :68-178; options :188-196)
 *   mpcx_solve_batch    sol = solver(x0=, lbx=, ubx=, lbg=, ubg=, p=)
 *                         Casadi/multiple_shooting_casadi.py:235-242, batched
 *                         over B independent parameter vectors p
 *   mpcx_plant_step     state_init = F(args['p'], u[:, 0])[0]
 *                         Casadi/multiple_shooting_casadi.py:273 (F built at :98-114)
 *   mpcx_rk4_sens       the function + derivative evaluations IPOPT requests from
 *                         CasADi inside solver() (F and its AD, :157 / :197):
 *                         kernel-level entry of the RK4 + Jacobian sweep
 *   mpcx_destroy        (Python garbage collection of the solver object)
 *   mpcx_last_error     (CasADi raises RuntimeError; here: message of the last
 *                         failing call on this thread)
 *
 * Conventions.  All arithmetic is IEEE fp64.  Pointers named d_* are device
 * pointers (hipMalloc'ed or torch CUDA tensors); everything else is host memory.
 * Functions return 0 on success and a negative mpcx_err code on error.  Host
 * calls are synchronous.  A handle is owned by one host thread at a time.
 *
 * Decision-vector layout = the reference's interleaved w (:128-170):
 *   w = [X_0(nx) | U_0(nu) X_1(nx) | ... | U_{N-1}(nu) X_N(nx)],  n_w = nx + N(nu+nx)
 * Constraint layout (:131,:172-175), all equalities (lbg = ubg = 0):
 *   g = [P[:nx] - X_0 ; F(X_k,U_k).xf - X_{k+1}  (k = 0..N-1)],  n_g = nx (N+1)
 */
#ifndef MPCX_H_
#define MPCX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpcx_handle mpcx_handle;

enum mpcx_model {
  MPCX_MODEL_UNICYCLE = 1, /* x=(x,y,theta), u=(v,omega): Casadi/multiple_shooting_casadi.py:68-72 */
  /* x+ = A_j x + B_j u + c_j, l = (z - zr_k)^T W_j (z - zr_k), z = (x, u): the mpctools
     LTI/LTV QPs (Inverted_pendulum/inverted_pendulum_single_shooting_mpctools.py:19-64,
     Trajectory Tracking/Trajectory_tracking_dynamic_model.py:117-145); tables set with
     mpcx_set_linear_model.  (nx, nu) in {(4,1), (5,1), (4,2)}; smaller models
     embed with zero pad states (mpcx/lti.py StatePad). */
  MPCX_MODEL_LINEAR = 2,
  /* Nonlinear ODE models (BASELINE config variants; parity against the CPU oracle only),
     RK4 with M substeps, node cost l = sum Q_i (x_i - xr_i)^2 + sum R_j (u_j - ur_j)^2,
     exact derivatives (mpc-verde_amd/csrc/ode.h).  Constants in mpcx_spec.par. */
  MPCX_MODEL_KIN_BICYCLE = 3, /* x=(X,Y,psi), u=(v,delta); par = (L) */
  MPCX_MODEL_DYN_BICYCLE = 4, /* x=(X,Y,psi,vx,vy,r), u=(delta,ax), linear tyres; par = (m,a,b,Ca,Jz):
                                 the nonlinear parent of Trajectory_tracking_dynamic_model.py:119-128 */
  MPCX_MODEL_CARTPOLE = 5,    /* x=(p,p',phi,phi'), u=F; par = (M,m,L,g,c): the nonlinear parent of
                                 inverted_pendulum_single_shooting_mpctools.py:19-23 */
  /* Path-frame kinematic bicycle with steering-rate limits (Trajectory Tracking/test2.py:103-112,42-59):
     x=(y,phi,v,s), u=(d,a); s = the steering applied in the previous interval (s_0 = delta_prev in x0),
     d = its increment, delta = s + d held over the interval and s+ = delta exactly, so the script's Du
     bound is lbu/ubu[0] and its steering bound lbx/ubx[3].  Stage rows (MPCX_P_X0_STAGEREF only)
     (yt, phit, vdes, kappa, d_ref, a_ref): yt, phit and the curvature kappa enter the dynamics
       y' = v sin(phi-phit), phi' = v (c2 tan(c1 delta) - kappa cos(phi-phit)/(1-(y-yt) kappa)), v' = a;
     the node cost is the diagonal one against (yt, phit, vdes, -, d_ref, a_ref) (Q[3] weighs s itself)
     plus w_z (tan(delta) - L kappa)^2.  par = (L, c1, c2, w_z): (c1, c2) = (1, 1/L) the bicycle,
     (1/L, 1) the script's tan(delta/L) (:109).  The value 6 stays unassigned: callers of earlier
     versions, and the library's own argument-checking suite, know it as an unknown model. */
  MPCX_MODEL_PATH_BICYCLE = 7
};

enum mpcx_cost {
  /* J = sum_k RK4 quadrature of L over [t_k, t_k+T] (Casadi/multiple_shooting_casadi.py:98-113) */
  MPCX_COST_QUADRATURE = 0,
  /* J = sum_k l(x_k, u_k, p_k) at the shooting nodes (mpctools nmpc;
     Trajectory Tracking/Trajectory_tracking.py:57-61) */
  MPCX_COST_NODE = 1
};

enum mpcx_param_layout {
  /* p = [x0 (nx); x_ref (nx)]  (n_p = 2 nx, Casadi/multiple_shooting_casadi.py:74,228-231) */
  MPCX_P_X0_XREF = 0,
  /* p = [x0 (nx); (x_ref_k, u_ref_k) for k = 0..N-1]  (n_p = nx + N (nx+nu);
     Trajectory Tracking/Trajectory_tracking.py:84-97,105-106).  Always used by
     MPCX_MODEL_LINEAR (z_ref_k = (x_ref_k, u_ref_k)). */
  MPCX_P_X0_STAGEREF = 1
};

enum mpcx_status {
  MPCX_CONVERGED = 0,   /* optimality error <= tol and the unscaled tests hold (IPOPT "Solve_Succeeded") */
  MPCX_ACCEPTABLE = 1,  /* acceptable level for acceptable_iter iterations, or an acceptable point at a
                           failed line search ("Solved_To_Acceptable_Level") */
  MPCX_MAX_ITER = 2,    /* iteration limit reached */
  MPCX_FAILED = 3,      /* line search failed and could not be recovered ("Restoration_Failed") */
  MPCX_INFEASIBLE = 4,  /* the restoration phase converged to a point of local infeasibility
                           ("Infeasible_Problem_Detected") */
  MPCX_STEP_FAILED = 5  /* inertia correction failed ("Error_In_Step_Computation") */
};

enum mpcx_err {
  MPCX_OK = 0,
  MPCX_EINVAL = -1,  /* bad argument (message via mpcx_last_error) */
  MPCX_EHIP = -2,    /* HIP runtime error */
  MPCX_ENOMEM = -3
};

typedef struct mpcx_spec {
  int32_t model;        /* mpcx_model */
  int32_t cost;         /* mpcx_cost */
  int32_t param_layout; /* mpcx_param_layout */
  int32_t N;            /* horizon (intervals), 1..255 (N >= 64: one workgroup of 128/256 lanes per instance) */
  int32_t M;            /* RK4 substeps per interval (M at :101; mpctools M at Trajectory_tracking.py:51) */
  int32_t max_iter;     /* IPOPT max_iter (:190) */
  int32_t device;       /* HIP device ordinal */
  int32_t group_policy; /* lanes per instance: 0 = widen (up to 64) while the batch leaves SIMDs idle,
                           1 = the smallest power of two >= N+1 (the same bits either way; see
                           mpcx_launch_shape) */
  double T;             /* sampling time (:31) */
  double tol;           /* IPOPT tol (default 1e-8) */
  double Q[8];          /* diagonal state weights (:78-83) */
  double R[8];          /* diagonal control weights (:81-84) */
  double lbu[8], ubu[8];/* control bounds (:42-45) */
  double lbx[8], ubx[8];/* state bounds (+-1e20 = free; Trajectory_tracking.py:64-67) */
  /* Warm start (IPOPT warm_start_init_point = yes), used when multipliers are
     passed in (lam_g0 / lam_x0 != NULL): initial barrier parameter, primal bound
     push and bound-multiplier push.  Defaults 1e-4. */
  double warm_mu_init, warm_bound_push, warm_mult_push;
  int32_t nx, nu;       /* state / control dimensions (unicycle: 3, 2) */
  double par[8];        /* model constants of the ODE models (see mpcx_model) */
  /* IPOPT termination and recovery options (IPOPT's names and semantics; the reference passes
     max_iter, acceptable_tol = 1e-8 and acceptable_obj_change_tol = 1e-6 at
     Casadi/multiple_shooting_casadi.py:188-196).  A field left 0 takes IPOPT's default:
     dual_inf_tol 1, constr_viol_tol 1e-4, compl_inf_tol 1e-4 (unscaled tests next to tol),
     acceptable_tol 1e-6, acceptable_dual_inf_tol 1e10, acceptable_constr_viol_tol 1e-2,
     acceptable_compl_inf_tol 1e-2, acceptable_obj_change_tol 1e20, acceptable_iter 15 (-1
     disables the acceptable-level termination).  IPOPT's literal acceptable_obj_change_tol = 0
     is expressed as the smallest positive double (4.9e-324, the same test); a negative value
     also selects the default.  mpcx_default_spec fills every field: the unicycle gets
     the reference script's acceptable_tol 1e-8 / acceptable_obj_change_tol 1e-6 (the problem of
     :181-197 as the script builds it), the ODE models IPOPT's defaults.  (mpcx.nlpsol without
     options uses IPOPT's defaults for every model, as ca.nlpsol without options does.)
     ABI change (round 4): acceptable_obj_change_tol = 0 used to be taken literally; it now
     selects the default like every other 0 field (write 4.9e-324 for IPOPT's literal 0). */
  double dual_inf_tol, constr_viol_tol, compl_inf_tol;
  double acceptable_tol, acceptable_dual_inf_tol, acceptable_constr_viol_tol, acceptable_compl_inf_tol;
  double acceptable_obj_change_tol;
  int32_t acceptable_iter;
  /* 0: a failed line search enters IPOPT's soft restoration and then the feasibility
     restoration phase (models that have one: the ODE models); 1: the solve ends there
     (MPCX_FAILED unless the point is acceptable) */
  int32_t no_restoration;
} mpcx_spec;

/* Fill *s with the reference's constants for model/cost at horizon N
   (unicycle point-to-point: T=0.2, M=4, Q=diag(1,5,0.1), R=diag(0.5,0.05),
   |v|<=1, |omega|<=pi/4, max_iter=2000, tol=1e-8).  ODE models: node cost, M=1,
   param_layout MPCX_P_X0_STAGEREF (cart-pole: MPCX_P_X0_XREF), the constants listed
   at mpcx_model and the defaults of mpcx/ode.py.  MPCX_MODEL_PATH_BICYCLE: the constants of
   Trajectory Tracking/test2.py (T=0.05, L=3.5, Q=(1.75,2.5,2.5,0)/(N+1), R=(0,0.4)/(N+1),
   w_z=10/(N+1), |s|<=0.384, |d|<=0.1225, |a|<=2; :19-59) with the bicycle form of the steering term. */
int mpcx_default_spec(mpcx_spec* s, int32_t model, int32_t N);

int mpcx_create(const mpcx_spec* s, mpcx_handle** h);
void mpcx_destroy(mpcx_handle* h);
const char* mpcx_last_error(void);
/* Build identity: a hash of the sources the library was compiled from (no reference
   counterpart; mpcx/_lib.py refuses a libmpcx.so whose hash differs from the tree's). */
const char* mpcx_source_hash(void);

/* Tables of an MPCX_MODEL_LINEAR handle (host pointers, copied to the device):
 *   A n_tab x nx x nx, B n_tab x nx x nu, c n_tab x nx (may be NULL = 0),
 *   W n_tab x nz(nz+1)/2 packed upper triangle of the stage weight (nz = nx+nu),
 *   tab tab_rows x N int32 table index of each stage; tab_rows = 1 (shared by all
 *   instances) or >= the batch size (row b = instance b; LTV schedules).
 * Call before solving; may be called again (e.g. per closed-loop step).
 * Reproducibility: with shared tables whose stages end in a decoupled suffix (B = 0, no x-u
 * weight; the move-blocked cart-pole QP), a launch may find the suffix's value functions cached
 * by an earlier launch of this handle; a factorisation that computes them afresh is redone on the
 * path the cached ones take, so results are bit-identical whatever the cache state (fresh handle,
 * cached handle, a later step of a multi-step launch). */
int mpcx_set_linear_model(mpcx_handle* h, int32_t n_tab, const double* A, const double* B, const double* c,
                          const double* W, const int32_t* tab, int32_t tab_rows);

/* Device-resident stage schedule (LTV closed loops: advance the table index of every
 * instance on the device each step without re-uploading tables).  d_tab is a caller-owned
 * device array tab_rows x N int32 with the meaning of `tab` above; it must stay valid while
 * the handle solves.  Indices outside [0, n_tab) are clamped.  d_tab = NULL reverts to the
 * schedule given to mpcx_set_linear_model (which also clears this one). */
int mpcx_set_linear_tab_dev(mpcx_handle* h, const int32_t* d_tab, int32_t tab_rows);

/* Device-resident box bounds per instance (fleets with different actuator limits, per-vehicle
 * corridors).  d_lbw and d_ubw are caller-owned device arrays n_steps x rows x n_w in the
 * interleaved w layout, +-1e20 = no bound; rows = 1 (one row shared by the batch) or >= the batch
 * size of every later launch (row b = instance b; a launch with more instances than rows returns
 * MPCX_EINVAL and launches nothing).  The X_0 entries (index < nx) are never read.
 * Precedence at a launch: the lbw / ubw arguments of mpcx_solve_batch, then the bounds installed
 * here, then the spec's.  n_steps = 1 gives the same bounds at every closed-loop step.  With
 * n_steps > 1 the array holds one block per step (a corridor that moves with time):
 * mpcx_solve_batch_dev, mpcx_step_dev and mpcx_solve_batch read block 0, and a lock-step loop
 * installs each step's block before the step (the setter on d_lbw + s rows n_w, n_steps = 1).
 * mpcx_run_dev loads an instance's bounds once, at the start of the launch, and returns
 * MPCX_EINVAL while bounds with n_steps > 1 are installed: reloading them at every step boundary
 * inside the kernel cost the 20-step unicycle launch 7 % (profiles/instance_bounds/).
 * Lifetime: the arrays must stay valid and unchanged while installed; after changing their
 * contents call the setter again (it validates them and decides which kernel variant a launch
 * runs).  Both pointers NULL reverts to the spec bounds; exactly one NULL is MPCX_EINVAL.
 * Validation runs on the device, on `stream`: NaN, lb > ub, or lb == ub finite (a fixed
 * variable) at an index >= nx returns MPCX_EINVAL, the message naming step, row and index of
 * the first such entry, and leaves the handle's bounds as they were.  The call reads the result
 * back, so it waits for `stream` and cannot be captured in a graph. */
int mpcx_set_bounds_dev(mpcx_handle* h, const double* d_lbw, const double* d_ubw, int32_t rows, int32_t n_steps,
                        void* stream);

/* n_w, n_g, n_p of the NLP described by the handle. */
int mpcx_dims(const mpcx_handle* h, int32_t* n_w, int32_t* n_g, int32_t* n_p);

/* Diagnostic environment knobs (A/B of two code paths; never needed in production):
 *   MPCX_DEC_SUFFIX=0           read by mpcx_set_linear_model: no decoupled-suffix reuse (the full Riccati
 *                               recursion at every factorisation; with it, config 5 at N >= 64 sums
 *                               the suffix's vector part in chain order: ~1e-12 relative, same
 *                               iteration counts)
 *   MPCX_UNICYCLE_SCAN_MIN_N=n  read once per process: the unicycle horizon from which the Riccati recursion runs as
 *                               the log-depth scan (default 25; 256 = never; ~1e-12 relative)
 *
 * The solve kernel a batch of B instances runs on this handle's device (no device work; no
 * reference counterpart -- it names what the profiler will show):
 *   lanes     lanes per instance group G (16, 32, 64, 128, 256; > 64 = one workgroup per instance)
 *   replicas  1, or 2 when a batch too small to give every SIMD a wave widens a 32-lane group to
 *             a wave and holds it twice, one replica per half-wave (group_policy 0)
 *   kernel    the kernel's demangled name as rocprofv3 prints it (may be NULL), e.g.
 *             "void mpcx::solve_kernel<mpcx::UnicycleFreeModel, 32, false, 2>(mpcx::SolveArgs)";
 *             kernel_len = buffer size (EINVAL if too small)
 * Batch-size dependence of the results: NONE.  Every group variant (narrow, widened, replicated,
 * multi-wave) gives an instance the same bits, whatever batch, group_policy or device (SIMD count)
 * it is solved with, so a global batch sharded over ranks returns what one device returns. */
int mpcx_launch_shape(const mpcx_handle* h, int32_t B, int32_t* lanes, int32_t* replicas, char* kernel,
                      int32_t kernel_len);

/* Batched NLP solve (host pointers, synchronous).
 *   P      B x n_p parameters (layout per spec.param_layout)
 *   w0     B x n_w initial guesses, or NULL = cold start (X_k = x0, U_k = 0: the
 *          feasible guess X0 = repmat(state_init), u0 = zeros that the script builds at
 *          :212-213; its own first solve passes the all-zero w0 of :118-169, which equals
 *          this guess for its state_init = 0, and later solves pass the shifted guess)
 *   lam_g0 B x n_g, lam_x0 B x n_w: initial multipliers (CasADi's lam_g0 /
 *          lam_x0 solver inputs), or NULL.  If either is given the solve starts
 *          as IPOPT's warm_start_init_point (spec.warm_*); otherwise as IPOPT's
 *          default (mu = 0.1, multipliers 0 / 1).
 *   lbw/ubw n_w bound vectors shared by the batch, or NULL = spec bounds
 *          (the reference's lbx/ubx, :199-206; X_0 is always free: it is
 *          pinned by the lifted constraint g_0 = x0 - X_0 and enters nothing else --
 *          interval 0 integrates from the parameter x0, F(x0=[P[:nx]; ...], p=U_0),
 *          as the script does at :125,157, so lam_g[0:nx] is 0 at a solution: exactly
 *          from a start without multipliers, to the dual tolerance from a warm one)
 *   w_out  B x n_w optimal decision vectors (interleaved reference layout)
 *   f_out  B objective values, or NULL
 *   g_out  B x n_g constraint values at w_out, or NULL
 *   lam_g  B x n_g constraint multipliers (CasADi sign convention), or NULL
 *   lam_x  B x n_w bound multipliers (CasADi convention: z_U - z_L), or NULL
 *   status B mpcx_status codes, or NULL
 *   iters  B iteration counts, or NULL                                        */
int mpcx_solve_batch(mpcx_handle* h, int32_t B, const double* P, const double* w0, const double* lam_g0,
                     const double* lam_x0, const double* lbw, const double* ubw, double* w_out, double* f_out,
                     double* g_out, double* lam_g, double* lam_x, int32_t* status, int32_t* iters);

/* Device-pointer variant: all work is enqueued on `stream` (a hipStream_t, NULL = default
   stream).  Any d_* except d_P and d_w_out may be NULL.  The handle owns scratch buffers that
   every launch of the handle uses (restoration workspace, cached suffix value functions), so a
   handle must not be used on two streams concurrently (one handle per stream, as per thread).
   The first call at a batch size larger than any before grows the restoration workspace: that
   call waits for the device to go idle (an earlier launch may still read the old buffer) and is
   therefore not capturable in a graph; later calls never synchronise. */
int mpcx_solve_batch_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w0, const double* d_lam_g0,
                         const double* d_lam_x0, double* d_w_out, double* d_f_out, double* d_lam_g,
                         double* d_lam_x, int32_t* d_status, int32_t* d_iters, void* stream);

/* Plant / integrator F (host): xf = F(x0, u).xf, qf = F(x0, u).qf for B
   instances; P as in mpcx_solve_batch (only x0 and the stage-0 reference are
   read), u B x nu.  qf may be NULL. */
int mpcx_plant_step(mpcx_handle* h, int32_t B, const double* P, const double* u, double* xf, double* qf);

/* Receding-horizon update on the device (one closed-loop step of
   Casadi/multiple_shooting_casadi.py:271-287): x0 <- F(x0, u_0*) in d_P, and
   d_w0_next = the optimal w shifted by one interval (last interval repeated).
   If d_lam_g / d_lam_x are given, the multipliers are shifted the same way into
   d_lam_g0_next / d_lam_x0_next (warm start of the next solve). */
int mpcx_shift_dev(mpcx_handle* h, int32_t B, double* d_P, const double* d_w, double* d_w0_next,
                   const double* d_lam_g, double* d_lam_g0_next, const double* d_lam_x, double* d_lam_x0_next,
                   void* stream);

/* One closed-loop step on the device in ONE kernel launch: the batched solve of
 * mpcx_solve_batch_dev followed, in the same kernel, by the receding-horizon update of
 * mpcx_shift_dev (identical results), written IN PLACE:
 *   d_P[:, 0:nx]  <- F(x0, u_0*)                      (plant, :273)
 *   d_w0          <- solution shifted by one interval  (warm start of the next step)
 *   d_lam_g0/d_lam_x0 <- multipliers shifted alike (may be NULL: not kept)
 * flags: MPCX_STEP_COLD -- ignore d_w0 / multipliers on input (cold start, see w0 above);
 *        MPCX_STEP_PRIMAL_ONLY -- warm primal start, default multiplier initialisation.
 * Otherwise the solve starts from d_w0 and (if given) the shifted multipliers as IPOPT's
 * warm_start_init_point.  Solution outputs as in mpcx_solve_batch_dev (d_w_out required). */
enum mpcx_step_flags { MPCX_STEP_COLD = 1, MPCX_STEP_PRIMAL_ONLY = 2 };
int mpcx_step_dev(mpcx_handle* h, int32_t B, double* d_P, double* d_w0, double* d_lam_g0, double* d_lam_x0,
                  int32_t flags, double* d_w_out, double* d_f_out, double* d_lam_g, double* d_lam_x,
                  int32_t* d_status, int32_t* d_iters, void* stream);

/* K closed-loop steps in ONE launch: every instance runs its own receding-horizon loop
 * (solve, plant, shift, warm restart -- exactly the sequence of K mpcx_step_dev calls, with
 * bit-identical results) without waiting for the other instances between steps; instances
 * are independent, so this changes no result, only how long the slowest solves hold the
 * batch.  Arguments as mpcx_step_dev, plus:
 *   K         number of steps (>= 1)
 *   d_Pseq    K x B x n_p stage references of every step (row s used from step s >= 1,
 *             the x0 columns are ignored; row 0 must match d_P) or NULL = d_P's for all
 *   d_tabseq  K x B x N linear-model schedules per step (row s from step s >= 1) or NULL
 *   d_status, d_iters  K x B (step-major).
 * On return d_P / d_w0 / d_lam_g0 / d_lam_x0 hold the state after step K (as after K
 * mpcx_step_dev calls) and d_w_out / d_f_out / d_lam_g / d_lam_x step K's solution. */
int mpcx_run_dev(mpcx_handle* h, int32_t B, int32_t K, double* d_P, double* d_w0, double* d_lam_g0, double* d_lam_x0,
                 int32_t flags, const double* d_Pseq, const int32_t* d_tabseq, double* d_w_out, double* d_f_out,
                 double* d_lam_g, double* d_lam_x, int32_t* d_status, int32_t* d_iters, void* stream);

/* RK4 + Jacobian sweep over B x N shooting intervals (host pointers).
 *   w      B x n_w decision vectors (interleaved layout)
 *   P      B x n_p parameters
 * Outputs, per instance b and interval k (row-major, k fastest after b):
 *   c      B x N x nx   defects F(X_k,U_k).xf - X_{k+1}
 *   q      B x N        F(X_k,U_k).qf
 *   A      B x N x nx x nx   dF.xf/dX_k
 *   Bm     B x N x nx x nu   dF.xf/dU_k
 *   gq     B x N x (nx+nu)   dF.qf/d(X_k,U_k)                               */
int mpcx_rk4_sens(mpcx_handle* h, int32_t B, const double* w, const double* P, double* c, double* q, double* A,
                  double* Bm, double* gq);

/* Device variant of the sweep on tiled structure-of-arrays buffers (the layout the
   kernel streams from HBM).  Instances are grouped in T = ceil(B/64)
   tiles of 64; an array with S stages and F fields per stage holds element
   (stage s, field i, instance b) at  ((s*T + b/64)*F + i)*64 + b%64  (size S*T*F*64):
 *   d_X  S=N+1, F=nx;  d_U  S=N, F=nu;  d_xr  S=1, F=nx          (inputs)
 *   d_J  S=N, 24 fields per interval: 0-2 c (defect), 3 q, 4-12 A (row-major),
 *        13-18 Bm (row-major), 19-23 gq (output), stored as 12 field PAIRS so that a lane
 *        writes 16 B: field f of (stage s, instance b) at
 *        (((s*T + b/64)*12 + f/2)*64 + b%64)*2 + f%2   (size N*T*24*64) */
int mpcx_rk4_sens_dev(mpcx_handle* h, int32_t B, const double* d_X, const double* d_U, const double* d_xr,
                      double* d_J, void* stream);

/* Sensitivities of the solution to the initial state x0 = P[:nx] (the MPC feedback gain), at a
 * primal-dual point (w, lam_g, lam_x) as a solve returns it -- no reference counterpart.
 * With H_k the exact Lagrangian Hessian of stage k, A_k, B_k its Jacobians (stage 0 at (x0, U_0)),
 *   Sigma_i = zL_i / (w_i - lbw_i) + zU_i / (ubw_i - w_i),  zU = max(lam_x, 0), zL = max(-lam_x, 0)
 * on the finitely bounded variables (0 elsewhere; X_0 is free), one backward Riccati sweep on
 * H + Sigma, A, B from P_N = Sigma_x (no regularisation) gives the gains K_k, with
 * K_0 = -Huu'_0^-1 (Hux_0 + B_0^T P_1 A_0), and
 *   Phi_0 = I,  Phi_{k+1} = (A_k + B_k K_k) Phi_k,   dX_k/dx0 = Phi_k,   dU_k/dx0 = K_k Phi_k,
 * followed by one step of iterative refinement on that linear system (residuals in twice the
 * working precision), so the result holds to a few ulps also where the open loop is unstable.
 * These are the sensitivities of the BARRIER problem at the multipliers passed in: at a solution
 * they approach the active-set sensitivities (active variables fixed) as mu -> 0 under strict
 * complementarity; a weakly active bound gives a value between the two one-sided derivatives.
 *   dw_dx0  B x n_w x nx, row = index in w (the dX_0/dx0 rows are exactly the identity), or NULL
 *   K0      B x nu x nx = dU_0/dx0, rows nx..nx+nu of dw_dx0 (the same bits): u ~ u0* + K0 (x - x0);
 *           or NULL.  At least one of dw_dx0 / K0 must be given.
 *   flag    B: 0 regular; 1 irregular -- a finitely bounded variable without positive slack, or a
 *           stage whose reduced Huu' is not positive definite (the derivative of a regularised
 *           system would be that of another problem, so none is applied).  An irregular instance
 *           gets NaN in all its outputs; the other instances are unaffected and the call returns 0.
 *           May be NULL.
 * Bounds: the precedence of a solve launch -- the host call's own lbw / ubw, then the arrays
 * installed by mpcx_set_bounds_dev (block 0), then the spec's.  Horizons N >= 64 (lane groups wider
 * than a wavefront) return MPCX_EINVAL, as do B <= 0, a NULL required pointer and both outputs
 * NULL; nothing is launched then.  An instance's bits do not depend on the batch it is in.
 * The device variant only enqueues one launch on `stream`: it never synchronises, allocates nothing
 * and can be captured in a graph. */
int mpcx_sens_x0_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                     const double* d_lam_x, double* d_dw_dx0, double* d_K0, int32_t* d_flag, void* stream);
int mpcx_sens_x0(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                 const double* lam_x, const double* lbw, const double* ubw, double* dw_dx0, double* K0,
                 int32_t* flag);

/* Directional sensitivities of the solution to the whole parameter row -- x0 and the target x_ref
 * (MPCX_P_X0_XREF) or the stage references (x_ref_k, u_ref_k) (MPCX_P_X0_STAGEREF) -- at a primal-dual
 * point as a solve returns it: dw = (dw* / dP) dP for m directions dP, each shaped like a row of P.
 * One launch, no solve; no reference counterpart.  Along a direction dp the KKT matrix is that of
 * mpcx_sens_x0 (H_k + Sigma_k, A_k, B_k, stage 0 with its feedback, P_N = Sigma_x) and the right-hand
 * side is dX_0 = dp[:nx] and, per stage k < N,
 *   r_k = d(grad_{z_k} l_k)/dp . dp,  l_k = q_k + lam_{k+1}^T f_k   (node cost: -2 W (dx_ref_k, du_ref_k)),
 *   d_k = d f_k/dp . dp                                            (0 for every supported model).
 * Backward from p_N = 0: s = p_{k+1} + P_{k+1} d_k, gu = r^u_k + B_k^T s, kf_k = -Huu'_k^-1 gu,
 * p_k = r^x_k + A_k^T s + K_k^T gu; forward: dU_k = K_k dX_k + kf_k, dX_{k+1} = A_k dX_k + B_k dU_k + d_k;
 * then one step of iterative refinement on the full system (residuals in twice the working precision).
 * With the x0 part alone the result is mpcx_sens_x0's to rounding; the first-order predictor of a
 * parameter change is w(P + dP) ~ w + dw.  Barrier-problem sensitivities, as for mpcx_sens_x0.
 *   dP    B x m x n_p: m directions per instance, 1 <= m <= nx per call (more: several calls)
 *   dw    B x n_w x m, row = index in w, column = direction (the dX_0 rows are exactly dP[:, :, :nx];
 *         rows nx..nx+nu are dU_0).  A column's bits do not depend on the other columns or on m, nor
 *         an instance's on the batch it is in.
 *   flag  B: 0 regular, 1 irregular (as mpcx_sens_x0: NaN in all the instance's outputs, the others
 *         unaffected, the call returns 0).  May be NULL.
 * Bounds: as mpcx_sens_x0.  MPCX_EINVAL, with nothing launched: a NULL handle, B <= 0, a NULL pointer
 * other than lbw / ubw / flag, m outside 1..nx, N >= 64, and MPCX_MODEL_PATH_BICYCLE (its stage rows
 * enter the dynamics).  The device variant only enqueues one launch on `stream`: it never
 * synchronises, allocates nothing and can be captured in a graph. */
int mpcx_sens_p_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                    const double* d_lam_x, const double* d_dP, int32_t m, double* d_dw, int32_t* d_flag,
                    void* stream);
int mpcx_sens_p(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                const double* lam_x, const double* lbw, const double* ubw, const double* dP, int32_t m, double* dw,
                int32_t* flag);

/* Adjoint sensitivities (reverse mode of mpcx_sens_p): gP = (dw* / dP)^T g for m cotangents g, each shaped
 * like a row of w -- the gradient of a scalar loss on the solution with respect to every entry of the
 * parameter row, x0 and the target or all stage references, from one launch; no solve, no reference
 * counterpart.  The KKT matrix of mpcx_sens_x0 is symmetric, so the transpose solve is mpcx_sens_p's
 * Riccati solve of right-hand sides with the same factors and the cotangent in their place:
 * rq_k = gX_k for k = 0..N (node N included), rr_k = gU_k, d = 0, from a zero start X~_0 = 0, no sign
 * flipped; then one step of iterative refinement, as mpcx_sens_p.  With its result (X~, U~, p~) and the
 * costates lam~_k = P_k X~_k + p~_k, for every direction (r_k, d_k, dx0) of mpcx_sens_p
 *   <g, dw> = lam~_0^T dx0 + sum_{k<N} ( z~_k^T r_k + lam~_{k+1}^T d_k ),   z~_k = (X~_k, U~_k),  lam~_0 = p~_0,
 * and with r_k = G_k dzr_k, d_k = D_k dzr_k (node costs: G_k = -2 W; D_k = 0 for every supported model)
 *   gP[:nx] = lam~_0,    gzr_k = G_k^T z~_k + D_k^T lam~_{k+1},
 *   MPCX_P_X0_STAGEREF:  gP[nx + nz k : nx + nz (k+1)] = gzr_k        (nz = nx + nu)
 *   MPCX_P_X0_XREF:      gP[nx : 2 nx] = sum_k gzr_k[:nx].
 * So <g, dw> = <gP, dP> for dw = mpcx_sens_p(dP), to rounding.  Barrier-problem sensitivities, as mpcx_sens_x0.
 *   gw    B x m x n_w: m cotangents per instance, 1 <= m <= nx per call (more: several calls)
 *   gP    B x m x n_p: row c of instance b is the gradient for cotangent c; every entry is written (those
 *         no stage owns as 0).  A cotangent's bits do not depend on the other cotangents or on m, nor an
 *         instance's on the batch it is in; a zero cotangent gives zeros, and one on the X_0 rows alone
 *         gives gP[:nx] = gX_0 exactly and zeros elsewhere.
 *   flag  B: 0 regular, 1 irregular (as mpcx_sens_x0: NaN in all the instance's outputs, the others
 *         unaffected, the call returns 0).  May be NULL.
 * Measured against the recursion restated in long double (one MI355X): within 2e-16 relative to
 * max(1, |entry|) on the linear test problems (tests/test_gpu_sens_vjp.py).
 * Bounds: as mpcx_sens_x0.  MPCX_EINVAL, with nothing launched: a NULL handle, B <= 0, a NULL pointer
 * other than lbw / ubw / flag, m outside 1..nx, N >= 64, and MPCX_MODEL_PATH_BICYCLE (its stage rows
 * enter the dynamics).  The device variant only enqueues one launch on `stream`: it never
 * synchronises, allocates nothing and can be captured in a graph. */
int mpcx_sens_vjp_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                      const double* d_lam_x, const double* d_gw, int32_t m, double* d_gP, int32_t* d_flag,
                      void* stream);
int mpcx_sens_vjp(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                  const double* lam_x, const double* lbw, const double* ubw, const double* gw, int32_t m, double* gP,
                  int32_t* flag);

/* Directional sensitivities of the solution to the box bounds lbw / ubw at a primal-dual point as a solve
 * returns it: dw = (dw* / dlbw) dlbw + (dw* / dubw) dubw for m pairs of directions, each shaped like w.
 * One launch, no solve, every model (MPCX_MODEL_PATH_BICYCLE included: no reference hook of the model is
 * involved); no reference counterpart -- it replaces central differences of whole solves under moved
 * bounds.  With the complementarity products zL_i (w_i - lbw_i) and zU_i (ubw_i - w_i) held fixed the
 * KKT matrix is that of mpcx_sens_x0 and the bounds enter the right-hand side alone,
 *   r_i = -(sigL_i dlbw_i + sigU_i dubw_i),  sigL_i = zL_i / (w_i - lbw_i),  sigU_i = zU_i / (ubw_i - w_i),
 * on every finitely bounded variable, the X rows of node N included; d_k = 0 and dX_0 = 0.  The solve is
 * mpcx_sens_p's (Riccati solve of right-hand sides, one step of iterative refinement).
 * zL = max(-lam_x, 0), zU = max(lam_x, 0) is the ONE-SIDED split of the returned multiplier zU - zL that
 * Sigma of mpcx_sens_x0 uses: at most one of sigL_i, sigU_i is non-zero.  On a two-sided box the far
 * side's own multiplier mu / slack is dropped: an O(mu) error at the solver's final mu (1e-9), like the
 * difference between barrier and active-set sensitivities, but 2.6e-2 at mu = 1e-3 in a CPU check where
 * the exact split gave 3e-10.  At a strictly active bound dw_i -> dbound_i; at an inactive one the effect
 * is O(mu).
 *   dlbw, dubw  B x m x n_w each, 1 <= m <= nx per call; entries on X_0's rows and where the bound lies
 *               beyond +-1e19 are ignored (not read)
 *   dw          B x n_w x m, mpcx_sens_p's layout (the X_0 rows are exact zeros).  A column's bits do not
 *               depend on the other columns or on m, nor an instance's on the batch it is in.
 *   flag        as mpcx_sens_p.
 * Bounds in force: as mpcx_sens_x0.  MPCX_EINVAL, with nothing launched: a NULL handle, B <= 0, a NULL
 * pointer other than lbw / ubw / flag, m outside 1..nx, N >= 64.  The device variant only enqueues one
 * launch on `stream`: it never synchronises, allocates nothing and can be captured in a graph. */
int mpcx_sens_bounds_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                         const double* d_lam_x, const double* d_dlbw, const double* d_dubw, int32_t m, double* d_dw,
                         int32_t* d_flag, void* stream);
int mpcx_sens_bounds(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                     const double* lam_x, const double* lbw, const double* ubw, const double* dlbw,
                     const double* dubw, int32_t m, double* dw, int32_t* flag);

/* Reverse mode of mpcx_sens_bounds: the gradients of a scalar loss on the solution with respect to every
 * entry of lbw and ubw, for m cotangents g shaped like w, from one launch; no reference counterpart (it
 * replaces 2 n_w finite-difference solves).  With z~ = (X~, U~) the adjoint solve of mpcx_sens_vjp
 * (rq_k = gX_k on every node, rr_k = gU_k, zero start, one refinement step),
 *   glbw_i = -sigL_i z~_i,   gubw_i = -sigU_i z~_i      (sigL, sigU: the one-sided split above),
 * so <g, dw> = <glbw, dlbw> + <gubw, dubw> for dw = mpcx_sens_bounds(dlbw, dubw), to rounding.
 *   gw          B x m x n_w, 1 <= m <= nx per call
 *   glbw, gubw  B x m x n_w each; every entry is written: 0 on X_0's rows and where there is no finite
 *               bound, NaN throughout for an irregular instance.  A cotangent's bits do not depend on the
 *               others or on m, nor an instance's on its batch; a zero cotangent gives zeros.
 *   flag        as mpcx_sens_p.
 * Bounds, refusals and the device variant: as mpcx_sens_bounds. */
int mpcx_sens_bounds_vjp_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                             const double* d_lam_x, const double* d_gw, int32_t m, double* d_glbw, double* d_gubw,
                             int32_t* d_flag, void* stream);
int mpcx_sens_bounds_vjp(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                         const double* lam_x, const double* lbw, const double* ubw, const double* gw, int32_t m,
                         double* glbw, double* gubw, int32_t* flag);

/* The cost weights as the sensitivity calls below see them: a stage's weight row has n_wt entries,
 * nx + nu for the models with a diagonal cost (MPCX_MODEL_UNICYCLE and the ODE models), ordered
 * (Q_0..Q_{nx-1}, R_0..R_{nu-1}), and nz (nz + 1) / 2 for MPCX_MODEL_LINEAR: the packed upper triangle of
 * a stage table in mpcx_set_linear_model's layout of W, nz = nx + nu of the handle. */
int mpcx_weight_dims(const mpcx_handle* h, int32_t* n_wt);

/* Replace the diagonal weights Q (nx) and R (nu) of the handle's cost; host only, nothing is launched.
 * Every later launch uses them, with results bit-identical to those of a handle created with these
 * weights in its spec (a launch takes its weights from the spec each time; nothing else keeps them).
 * MPCX_EINVAL, the handle unchanged: MPCX_MODEL_LINEAR (its weights are its tables:
 * mpcx_set_linear_model), a NULL argument, an entry that is not finite or is negative. */
int mpcx_set_weights(mpcx_handle* h, const double* Q, const double* R);

/* Directional sensitivities of the solution to the cost weights at a primal-dual point as a solve
 * returns it: dw = (dw* / dweights) dW for m directions of the weight rows.  One launch, no solve, every
 * model; no reference counterpart -- it replaces central differences of whole solves on handles with
 * perturbed weights.  Only the stage cost q_k depends on the weights, and linearly, so the KKT matrix is
 * that of mpcx_sens_x0 (H_k + Sigma_k, A_k, B_k, stage 0 at (x0, U_0), P_N = Sigma_x) and a direction
 * enters the right-hand side alone, per stage k < N,
 *   r_k = d(grad_z q_k)/d(weights) . dW_k,    d_k = 0,  dX_0 = 0,  nothing on node N.
 * Diagonal node costs (MPCX_COST_NODE, every ODE model): r_{k,i} = 2 dW_{k,i} e_{k,i} with e_k the
 * residual of the model's own cost gradient -- z_k minus its reference; for MPCX_MODEL_PATH_BICYCLE
 * (y - yt, phi - phit, v - vdes, s, d - d_ref, a - a_ref); its hook weight w_z = par[3] is no part of the
 * row.  Unicycle with MPCX_COST_QUADRATURE: grad q is exactly linear and homogeneous in (Q, R), and r_k is
 * the model's own gradient evaluated with the direction in the weights' place.  MPCX_MODEL_LINEAR:
 * r_k = 2 dW_k (z_k - zr_k) with dW_k symmetric, packed as in mpcx_weight_dims.  The solve is
 * mpcx_sens_p's (Riccati solve of right-hand sides, one step of iterative refinement).  These are
 * barrier-problem sensitivities, as mpcx_sens_x0's.
 *   dW     B x m x (per_stage ? N : 1) x n_wt, 1 <= m <= nx per call: one row per stage, or
 *          (per_stage = 0) one row used at every stage; a row that is the same at every stage gives the
 *          same bits either way.  Exact: a zero direction gives zeros.
 *   dw     B x n_w x m, mpcx_sens_p's layout (the X_0 rows are exact zeros).  A column's bits do not
 *          depend on the other columns or on m, nor an instance's on the batch it is in.
 *   flag   as mpcx_sens_p.
 * Bounds in force: as mpcx_sens_x0.  MPCX_EINVAL, with nothing launched: a NULL handle, B <= 0, a NULL
 * pointer other than lbw / ubw / flag, m outside 1..nx, N >= 64.  The device variant only enqueues one
 * launch on `stream`: it never synchronises, allocates nothing and can be captured in a graph. */
int mpcx_sens_weights_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                          const double* d_lam_x, const double* d_dW, int32_t per_stage, int32_t m, double* d_dw,
                          int32_t* d_flag, void* stream);
int mpcx_sens_weights(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                      const double* lam_x, const double* lbw, const double* ubw, const double* dW, int32_t per_stage,
                      int32_t m, double* dw, int32_t* flag);

/* Reverse mode of mpcx_sens_weights: the gradients of a scalar loss on the solution with respect to every
 * stage's weight row, and their sum over the stages, for m cotangents g shaped like w, from one launch; no
 * reference counterpart (it replaces 2 n_wt finite-difference solves on new handles).  With z~ = (X~, U~)
 * the adjoint solve of mpcx_sens_vjp (rq_k = gX_k on every node, rr_k = gU_k, zero start, one refinement
 * step), <g, dw> = sum_{k<N} z~_k^T r_k, so per stage
 *   diagonal costs:  gWk_{k,i} = 2 z~_{k,i} e_{k,i}
 *   packed W:        gWk_k[a,a] = 2 z~_a e_a,   gWk_k[a,b] = 2 (z~_a e_b + z~_b e_a)  (a < b)
 *   quadrature cost: gWk_{k,i} = z~_k^T grad q_k at the unit weight i
 * and <g, dw> = <gWk, dW> for dw = mpcx_sens_weights(dW, per_stage = 1), to rounding.  X~_0 = 0, so stage
 * 0's state weights get an exact zero from the node costs.  gW = sum_k gWk_k is the gradient for a
 * direction applied to every stage alike: for the diagonal models, with respect to the handle's Q, R.
 *   gw     B x m x n_w, 1 <= m <= nx per call
 *   gWk    B x m x N x n_wt or NULL;  gW  B x m x n_wt or NULL; one of them is required.  Every entry of
 *          those given is written, NaN throughout for an irregular instance.  A cotangent's bits do not
 *          depend on the others or on m, nor an instance's on its batch; a zero cotangent gives zeros.
 *   flag   as mpcx_sens_p.
 * Bounds, refusals and the device variant: as mpcx_sens_weights. */
int mpcx_sens_weights_vjp_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                              const double* d_lam_x, const double* d_gw, int32_t m, double* d_gWk, double* d_gW,
                              int32_t* d_flag, void* stream);
int mpcx_sens_weights_vjp(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                          const double* lam_x, const double* lbw, const double* ubw, const double* gw, int32_t m,
                          double* gWk, double* gW, int32_t* flag);

/* The model as the sensitivity calls below see it: a stage's model row has n_th entries.
 *   ODE models: the leading entries of mpcx_spec.par that the model reads --
 *     MPCX_MODEL_KIN_BICYCLE 1 (L), MPCX_MODEL_DYN_BICYCLE 5 (m, a, b, Ca, Jz), MPCX_MODEL_CARTPOLE 5 (M, m, L, g, c),
 *     MPCX_MODEL_PATH_BICYCLE 4 (L, c1, c2, w_z; L and w_z enter its cost, c1 and c2 its dynamics).
 *   MPCX_MODEL_LINEAR: nx nx + nx nu + nx, the stage's tables (A row-major, B row-major, c) in
 *     mpcx_set_linear_model's layout, nx and nu of the handle.
 *   MPCX_MODEL_UNICYCLE: 0.  It has no constants; mpcx_set_par and the four sensitivity calls below return
 *     MPCX_EINVAL for it. */
int mpcx_model_dims(const mpcx_handle* h, int32_t* n_th);

/* Replace the constants par[0..n_th) of an ODE model's handle; host only, nothing is launched.  Every later
 * launch uses them, with results bit-identical to those of a handle created with these constants in its spec (a
 * launch takes them from the spec each time; nothing else keeps them).  MPCX_EINVAL, the handle unchanged:
 * MPCX_MODEL_LINEAR (its constants are its tables: mpcx_set_linear_model), MPCX_MODEL_UNICYCLE (none), a NULL
 * argument, an entry that is not finite, and for MPCX_MODEL_PATH_BICYCLE L = par[0] <= 0, as mpcx_create. */
int mpcx_set_par(mpcx_handle* h, const double* par);

/* Directional sensitivities of the solution to the model at a primal-dual point as a solve returns it:
 * dw = (dw* / dmodel) dTh for m directions of the model rows.  One launch, no solve; no reference counterpart --
 * it replaces central differences of whole solves on handles with perturbed constants or tables.  The KKT matrix
 * is that of mpcx_sens_x0 (H_k + Sigma_k, A_k, B_k, stage 0 at (x0, U_0), P_N = Sigma_x).  A model row th_k enters
 * the interval map F_k(z, th) and, for MPCX_MODEL_PATH_BICYCLE, the stage cost q_k(z, th).  Stationarity and
 * the defect of stage k are grad_z q_k + grad_z (lam_{k+1}^T F_k) - (lam_k; 0) = 0 and F_k - x_{k+1} = 0, so along
 * dTh_k, the multipliers held fixed, per stage k < N
 *   r_k = [d(grad_z q_k)/dth + d(grad_z (lam_{k+1}^T F_k))/dth] dTh_k,    d_k = (dF_k/dth) dTh_k,
 * dX_0 = 0, nothing on node N, and the linear system reads K (dz; dlam) + (r; d) = 0.  ODE models: r_k and d_k
 * come from hyper-dual RK4 passes with the constants seeded (exact: no truncation), nz passes per direction;
 * the 6-state bicycle runs its hyper-dual dynamics here.  MPCX_MODEL_LINEAR, closed form:
 *   d_k = dA_k x_k + dB_k u_k + dc_k  (x_0 = P[:nx]),    r_k = (dA_k^T lam_{k+1}; dB_k^T lam_{k+1}).
 * The solve is mpcx_sens_p's (Riccati solve of right-hand sides, one step of iterative refinement).  These are
 * barrier-problem sensitivities, as mpcx_sens_x0's.
 *   dTh    B x m x (per_stage ? N : 1) x n_th, 1 <= m <= nx per call: one row per stage, or (per_stage = 0) one
 *          row used at every stage (an ODE model's par); a row that is the same at every stage gives the same
 *          bits either way.  Exact: a zero direction gives zeros.
 *   dw     B x n_w x m, mpcx_sens_p's layout (the X_0 rows are exact zeros).  A column's bits do not depend on
 *          the other columns or on m, nor an instance's on the batch it is in.
 *   flag   as mpcx_sens_p.
 * Bounds in force: as mpcx_sens_x0.  MPCX_EINVAL, with nothing launched: a NULL handle, B <= 0, a NULL pointer
 * other than lbw / ubw / flag, MPCX_MODEL_UNICYCLE (n_th = 0), m outside 1..nx, N >= 64.  The device variant
 * only enqueues one launch on `stream`: it never synchronises, allocates nothing and can be captured in a graph. */
int mpcx_sens_model_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                        const double* d_lam_x, const double* d_dTh, int32_t per_stage, int32_t m, double* d_dw,
                        int32_t* d_flag, void* stream);
int mpcx_sens_model(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                    const double* lam_x, const double* lbw, const double* ubw, const double* dTh, int32_t per_stage,
                    int32_t m, double* dw, int32_t* flag);

/* Reverse mode of mpcx_sens_model: the gradients of a scalar loss on the solution with respect to every stage's
 * model row, and their sum over the stages, for m cotangents g shaped like w, from one launch.  K is symmetric
 * and the adjoint solve is mpcx_sens_vjp's, K (z~; lam~) + (g; 0) = 0 (rq_k = gX_k on every node, rr_k = gU_k,
 * d = 0, zero start, one refinement step), with lam~_k = P_k X~_k + p~_k its costates; lam~_{k+1} is the unknown
 * paired with stage k's defect row.  Then, no sign flipped,
 *   <g, dw> = sum_{k<N} (z~_k^T r_k + lam~_{k+1}^T d_k),
 *   gThk_k = (dr_k/dth_k)^T z~_k + (dd_k/dth_k)^T lam~_{k+1},
 * and <g, dw> = <gThk, dTh> for dw = mpcx_sens_model(dTh, per_stage = 1), to rounding.  ODE models: n_th nz
 * hyper-dual passes per instance and stage.  MPCX_MODEL_LINEAR: gA_k = lam~_{k+1} x_k^T + lam_{k+1} X~_k^T,
 * gB_k likewise with u_k and U~_k, gc_k = lam~_{k+1}.  gTh = sum_k gThk_k is the gradient for a row shared by
 * all stages: for the ODE models, with respect to the handle's par.
 *   gw     B x m x n_w, 1 <= m <= nx per call
 *   gThk   B x m x N x n_th or NULL;  gTh  B x m x n_th or NULL; one of them is required.  Every entry of those
 *          given is written, NaN throughout for an irregular instance.  A cotangent's bits do not depend on the
 *          others or on m, nor an instance's on its batch; a zero cotangent gives zeros.
 *   flag   as mpcx_sens_p.
 * Bounds, refusals and the device variant: as mpcx_sens_model. */
int mpcx_sens_model_vjp_dev(mpcx_handle* h, int32_t B, const double* d_P, const double* d_w, const double* d_lam_g,
                            const double* d_lam_x, const double* d_gw, int32_t m, double* d_gThk, double* d_gTh,
                            int32_t* d_flag, void* stream);
int mpcx_sens_model_vjp(mpcx_handle* h, int32_t B, const double* P, const double* w, const double* lam_g,
                        const double* lam_x, const double* lbw, const double* ubw, const double* gw, int32_t m,
                        double* gThk, double* gTh, int32_t* flag);

#ifdef __cplusplus
}
#endif

#endif /* MPCX_H_ */

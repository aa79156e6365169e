// ipm.h -- device-resident interior-point drivers behind solver().
//
//   Method::Hsd    homogeneous self-dual predictor-corrector, src/ipo/hsd.c:27-311
//   Method::Intpt  primal-dual path following,               src/ipo/intpt.c:33-261
//   Method::Hsdls  homogeneous self-dual long step,          src/ipo/hsdls.c:38-296
//   Method::Qp     intpt.c's path following with a quadratic objective term
//                  (an extension: the reference has no QP loop)
//   Method::Pc     Mehrotra's predictor-corrector on the same problems, LPs
//                  and convex QPs: one factorisation and two refined solves
//                  an iteration (an extension)
//
// The host keeps the handful of scalars the reference keeps (phi, psi, mu,
// theta, ...) and prints the reference's per-iteration trace; every O(m+n)
// vector, both SpMVs and the KKT factor/solve live on the GPU.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <memory>

#include "exchange.h"
#include "hip_util.h"
#include "kkt_device.h"
#include "row_ax.h"

namespace ipo {

enum class Method { Hsd = 0, Intpt = 1, Hsdls = 2, Qp = 3, Pc = 4 };

struct IpmOptions {
    Method method = Method::Hsd;
    int max_iter = 200;          // MAX_ITER, hsd.c:25 / intpt.c:31 (hsdls.c:25: 600)
    FILE* trace = nullptr;       // banner + one line per iteration, reference format
    bool timing = false;         // per-phase HIP-event timing
};

struct IpmResult {
    int status = 5;
    int iters = 0;
    double t_setup_s = 0.0;      // symbolic analysis + uploads (first ldltfac in the reference)
    double t_solve_s = 0.0;      // iteration loop, wall clock
    double final_mu = 0.0, final_pobj = 0.0, final_dobj = 0.0, final_pinf = 0.0, final_dinf = 0.0;
    double phi = 1.0, psi = 1.0;
    KktTimers kkt;
    long refine_passes = 0;
};

// One shard of a block-angular LP (not in the reference).
// The local problem holds this shard's diagonal blocks (rows, columns) and a
// replica of the nforced linking rows, numbered last.  Column quantities
// (x, z) are disjoint between shards, block-row quantities (y, w) too, and
// the linking-row values are replicated bitwise: every shard computes them
// from the same allreduced inputs.  Sums count linking rows on rank 0 only.
// nforced > 0 without an Exchange: one process, linking rows in the tail.
struct ShardSpec {
    int nforced = 0;              // linking rows = the last nforced local rows
    Exchange* xch = nullptr;      // not owned
    int m_global = 0, n_global = 0;
    long nz_global = 0;
};

// The slots of IpmSolver::scal_ (doubles on the device; the pinned hs_ takes
// its read-backs at the same indices unless a copy says otherwise).
// Slots 0 .. 4 are reused: every reduction writes its results there from
// kIsRed on, in its jobs' order.  The iteration's opening reduction of every
// method has the named dot products; the later ones of an iteration (the
// directions' c'fx, b'fy, c'gx, b'gy; two squared norms; one largest ratio)
// are read as kIsRed + k beside the job list that orders them.
constexpr int kIsRed = 0;
constexpr int kIsZx = 0, kIsWy = 1, kIsCx = 2, kIsBy = 3;   // z'x, w'y, c'x, b'y
constexpr int kIsXqx = 4;       // x'Qx (run_qp)
constexpr int kIsPhiMu = 6;     // [2] phi, mu as k_hsd_residuals reads them (k_hsd_mu)
constexpr int kIsNorm2 = 8;     // [2] squared norms of the primal and the dual residual
constexpr int kIsTheta = 11;    // the step length k_step reads (k_hsd_theta)
constexpr int kIsDphi = 12;     // [2] dphi, dpsi (k_hsd_dphi) for k_hsd_directions and k_hsd_theta
constexpr int kIsPhiNext = 14;  // [2] the next iteration's phi, psi (k_hsd_theta)
// run_pc (none of them is read back by the host):
constexpr int kIsPcRatio = 16;  // the predictor's largest ratio t (k_pc_affine)
constexpr int kIsPcDots = 17;   // [6] z'dxa, x'dza, w'dya, y'dwa, dxa'dza, dya'dwa (g1 and g2's terms)
constexpr int kIsPcMu = 23;     // the centring mu k_pc_rhs and k_pc_directions read (k_pc_mu)
// the Mehrotra start (IpmSolver::mehrotra_start; none of them is read back):
constexpr int kIsMsNegMin = 24; // [2] -min(x~, w~), -min(y~, z~) of the least-squares point (k_ms_unpack)
constexpr int kIsMsDelta = 26;  // [2] the shifts delta_p, delta_d (k_ms_delta)
constexpr int kIsMsSums = 28;   // [3] g = x'z + w'y, Sp = sum x + sum w, Sd = sum z + sum y (k_ms_shift)
constexpr int kIsMsEps = 31;    // [2] the balancing shifts eps_p, eps_d (k_ms_eps)
constexpr int kIsCount = 33;

// How a run of Intpt, Qp or Pc chooses its line 0 when no point is held:
// every variable 1000, or Mehrotra's least-squares point shifted into the
// interior and balanced, computed on the device from the
// problem's current numbers.
enum class StartRule { Default = 0, Mehrotra = 1 };

// Problem uploaded to HBM once; run() iterates from the reference's start
// point and can be called repeatedly (the bench times run()).
// bench.py's HBM-roofline leg: the HBM-bound HSD vector kernels timed alone
// (ipm_device.hip); out[3] ms per launch, bytes[3] algorithmic bytes per launch
void vector_bench(int m, int n, const int* kA, const int* iA, const double* A, int reps, double* out, double* bytes);

class IpmSolver {
  public:
    // q: the QP's Q (n x n, full symmetric CSC, positive semidefinite; its
    // qmax is not read): max c'x + f - x'Qx / 2.  With a nonempty Q the
    // solver runs Method::Qp and Method::Pc only, and cannot be sharded.
    IpmSolver(int m, int n, const int* kA, const int* iA, const double* A, const double* b, const double* c,
              double f, hipStream_t stream = nullptr, const ShardSpec* shard = nullptr, const QBlock* q = nullptr);
    ~IpmSolver();
    // Throws for an LP method on a solver built with a nonempty Q and for
    // Method::Qp or Method::Pc on a sharded solver.  Method::Qp without Q is
    // the QP with an empty Q: the LP, on the LP's factor.  Method::Pc runs on
    // solvers with and without Q.
    int run(const IpmOptions& opt, IpmResult* res);
    // copy x (n), y (m), w (m), z (n) of the last run to the host
    void download(double* x, double* y, double* w, double* z) const;
    KktDevice& kkt() { return *kkt_; }
    double setup_seconds() const { return t_setup_; }
    // New numbers on the constructor's pattern (ipo_hip_ctx_update; DESIGN.md
    // 10.3): each argument null (unchanged) or the full host array in the
    // constructor's layout, Q in q's kQ / iQ order.  The arrays given are
    // uploaded to staging buffers and validated there on the device (every
    // value finite, Q[k] == Q[its transposed entry]); only then are A and its
    // CSR copy, the RowAxPlan slices, Q and its diagonal, b, c and f replaced,
    // so after a throw (std::invalid_argument: a bad value, Q for a solver
    // without Q, a sharded solver) the solver runs with its old numbers.
    // The next run() sees what a solver constructed from the new arrays would.
    void update(const double* A, const double* b, const double* c, const double* f, const double* Q);
    // seconds of the last update(): the uploads with their validation, and the
    // device refresh that followed (both ended by a stream synchronisation)
    double update_upload_seconds() const { return t_upd_upload_; }
    double update_refresh_seconds() const { return t_upd_refresh_; }
    // The start point of the infeasible-start methods (Intpt, Qp, Pc) in place
    // of every variable 1000: host vectors x, z (n), y, w (m), every entry
    // finite and > 0 (checked on the device before the held start is
    // replaced; std::invalid_argument otherwise, and on a sharded solver).
    // All four null: back to the default.  It persists until cleared; Hsd and
    // Hsdls, whose state includes phi and psi, refuse to run while one is set.
    void set_start(const double* x, const double* y, const double* w, const double* z);
    // ... the iterate the last run() left, raised entry by entry to at least
    // floor > 0 (one kernel, no host round trip).  Throws before any run().
    void start_from_last(double floor);
    bool has_start() const { return has_start_; }
    // The rule for line 0 of Intpt, Qp and Pc.  The latest
    // call wins: setting a rule clears a held point, and set_start (its clear
    // call too) and start_from_last put the rule back to Default.  Under
    // Mehrotra every run() computes its start from the numbers then current
    // (one factorisation and two refined solves, counted in the run's time
    // and statistics); Hsd and Hsdls refuse to run.  Throws on a sharded solver.
    void set_start_rule(StartRule r);
    StartRule start_rule() const { return rule_; }
    // The rule's point for the current numbers into host vectors x, z (n), y,
    // w (m); Default: 1000 everywhere.  Changes nothing a later run() sees:
    // not the rule, a held start, the last iterate or the factor's eps_diag.
    void start_point(StartRule r, double* x, double* y, double* w, double* z);

  private:
    int run_hsd(const IpmOptions& opt, IpmResult* res);
    int run_intpt(const IpmOptions& opt, IpmResult* res);
    int run_hsdls(const IpmOptions& opt, IpmResult* res);
    int run_qp(const IpmOptions& opt, IpmResult* res);
    template <bool SW>
    int run_pc(const IpmOptions& opt, IpmResult* res);   // SW: the swapped factor of a solver with Q
    void reduce(const struct RedJobs& j, int nout);
    // sharded solve: linking-row products A_link x summed over the shards
    // into lax_ (no-op unsharded), and the cross-shard reduction of scalars
    void link_ax(const double* x);
    void xsum(double* d, size_t n, RedOp op) { if (xch_) xch_->allreduce(d, n, op, stream_); }
    // rows >= mrow() take A x from lax(): the summed linking rows of a shard,
    // or every row when A x is formed column-blocked (row_ax) beforehand
    const double* lax() const { return xch_ ? lax_.get() : axsliced_ ? ax_.get() : nullptr; }
    int mrow() const { return xch_ ? m_ - nforced_ : axsliced_ ? 0 : m_; }   // rows below are shard-local
    // A x of every row in column blocks whose x-slice fits one XCD's L2
    // (RowAxPlan, row_ax.h; bitwise the residual kernels' own sums), when x is
    // larger than a slice and the solver is not sharded
    void row_ax(const double* x, hipStream_t st);
    const KktKnobs knobs_ = KktKnobs::from_env();   // read once, at construction (kkt_knobs.h)
    bool axsliced_ = false;   // A x by RowAxPlan (rows_ax_sliced)
    DevBuf<double> ax_;
    RowAxPlan axplan_;
    void print_dims(FILE* tr) const;
    // x, z, y, w of a path-following run's line 0: the held start, the
    // rule's point, or v everywhere
    void init_point(double v, IpmResult* res);
    // Mehrotra's start into device vectors x, z (n), y, w (m); returns the
    // refinement passes of its two solves.  Leaves the factor of E = D = 1
    // behind and whatever eps_diag that factorisation grew to: the caller
    // puts eps_diag back.  Uses D_, E_, gx_, gy_, dx_, dy_, part_ and the
    // kIsMs slots.  Throws std::runtime_error if an entry came out not > 0.
    long mehrotra_start(double* x, double* y, double* w, double* z);
    void alloc_start();
    // the value maps of update() (value_maps.h), uploaded at construction
    int nz_ = 0, qnz_ = 0;
    DevBuf<int> ucsr_;           // has_q_: the factor's "A" (the CSR of A) from the caller's CSC
    DevBuf<int> qtmap_;          // has_q_: Q entry -> its transposed entry
    // update()'s staging (allocated by the first update that needs each)
    DevBuf<double> stA_, stAt_, stb_, stc_, stQ_;
    DevBuf<int> vfirst_;         // [kVfCount] first offending index of each validation
    double t_upd_upload_ = 0.0, t_upd_refresh_ = 0.0;
    // the start point: held (sx_ ...) and set_start()'s staging (tx_ ...)
    bool has_start_ = false, ran_ = false;
    StartRule rule_ = StartRule::Default;
    DevBuf<double> sx_, sy_, sw_, sz_, tx_, ty_, tw_, tz_;

    int m_, n_;
    double f_;
    hipStream_t stream_;
    bool own_stream_ = false;
    double t_setup_ = 0.0;
    int nforced_ = 0;
    Exchange* xch_ = nullptr;
    int mcnt_ = 0;               // rows this shard counts in sums (linking rows on rank 0 only)
    int mg_ = 0, ng_ = 0;        // global sizes (mu's denominator, the trace)
    int dot_segmin_ = 0;         // RedJobs::segmin of the solver's dots (dev_common.h)
    long nzg_ = 0;
    std::unique_ptr<KktDevice> kkt_;
    // a solver built with a nonempty Q: kkt_ is the factor with the roles of
    // x and y swapped, so that Q sits on KktDevice's first block (run_qp)
    bool has_q_ = false, sharded_ = false;
    DevBuf<double> qx_;          // Q x (n)
    DevBuf<double> b_, c_, x_, y_, w_, z_;
    DevBuf<double> rho_, sig_, D_, E_, fx_, fy_, gx_, gy_, dx_, dy_, dz_, dw_;
    DevBuf<double> part_, part2_, scal_, lax_;
    hipStream_t side_ = nullptr;            // mu / residuals beside the factorisation (run_hsd)
    hipEvent_t ev_step_ = nullptr, ev_side_ = nullptr;
    double* hs_ = nullptr;       // pinned scalars [kIsCount]
};

// Whole-pipeline convenience used by the C ABI: host arrays in, host out.
int ipm_solve_host(int m, int n, int nz, const int* iA, const int* kA, const double* A, const double* b,
                   const double* c, double f, double* x, double* y, double* w, double* z, const IpmOptions& opt,
                   IpmResult* res);

}  // namespace ipo

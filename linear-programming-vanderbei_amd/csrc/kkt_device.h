// kkt_device.h -- device-resident numeric LDL^T of the ipo KKT matrix.
//
// Replaces the numeric half of src/ipo/ldlt.c:
//   factor()   <- inv_num  ldlt.c:164-309 (assembly, lltnum :517-636,
//                 dependent-pivot rule :600-614, eps_diag growth :293-306)
//   solve()    <- solve    ldlt.c:327-425 (iterative refinement) with
//                 rawsolve ldlt.c:433-505 as supernodal level sweeps
// Everything stays in HBM between calls; only a few scalars (refinement
// residual, min |d|, dependent-pivot count) come back to the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "hip_util.h"
#include "exchange.h"
#include "kkt_flags.h"
#include "kkt_knobs.h"
#include "kkt_plan.h"
#include "kkt_schedule.h"

namespace ipo {

// Device view of the dense tail (see kkt_plan.h): S = nt x nt column-major.
// (kTailVisitBlocks, kTailVisitLatest: kkt_knobs.h; kTailSchedMaxBlocks: kkt_schedule.h)
struct TailView {
    double* S;
    int nt, ntb, tc;
    const int* task_ptr;
    const TailTask* tasks;
    double* W;        // nt x 64 workspace: L21 * D of the current block column
    int vk = kTailVisitBlocks;   // blocks per deferred trailing update (visit) of a tile
    int dep = 1;      // dependent pivots inside the look-ahead panel (kkt_dense.hip panel_w_body; 0: bail to the host)
    // visit schedule (tail_visit_schedule): launch t's visits are vlist[vptr[t] ..
    // vptr[t + 1]), each (bi | c << 8 | b0 << 16 | b1 << 24); vlist on the
    // device, vptr on the host; null: the visit_hi formula alone
    const unsigned* vlist = nullptr;
    const int* vptr = nullptr;
    int sdep = 1;     // dependent pivots inside the sparse fused panels (k_panel_w, k_panel_s; 0: redo the factor)
};

// The look-ahead dense tail as ONE persistent launch (k_tail_run): the
// items of launches [t0, ntb) of tail_run_schedule, drawn by ticket.
// Counters: pdone[t] = panel workgroups of step t done, vseq[bi * ntb + c] =
// visits of tile (bi, c) done -- both zeroed before a factorisation's first
// run and kept for a run resumed after a repair; ticket zeroed before every run.
struct TailRun {
    const uint2* items;   // the run's first item (launch t0's)
    int n;                // items in the run
    int t0;               // its first launch
    int* ticket;
    int* pdone;
    int* vseq;
    // [ntb] (null: off) panel workgroups of step t that held and have stored
    // everything of the step, workgroup 0's L11' included: tail_gp(nt, t) of
    // them make block column t readable while the run goes on (the trailing
    // forward lead, k_tail_fwd_lead<R, true>; never reached if a panel bails)
    int* cdone = nullptr;
    // window hand-off (kkt_dense.hip RunPub; null: off): tile window (t, j, w)
    // at pub + (((t & 1) ntb + j) 4 + w) kTailPubWin once wflag[(t ntb + j) 4
    // + w] == epoch (one epoch per launch, never reused: no reset)
    double* pub = nullptr;
    int* wflag = nullptr;
    int* pread = nullptr;     // [ntb] panels of step t done reading step t - 1's windows
    int epoch = 0;
    // developer trace (tools/ubench_tail UB_TRACE): per item {drawn, ready,
    // done} in s_memrealtime ticks (100 MHz) and the workgroup's XCC id; null: off
    unsigned long long* trace = nullptr;
};

// The run's counters in one allocation of words(ntb) ints: TailRun's ticket,
// pdone[ntb], vseq[ntb * ntb], pread[ntb] and cdone[ntb], then the trailing
// lead's ticket (launch_lead_trail), which the run's reset clears with them.
struct RunCounters {
    static constexpr size_t kTicket = 0, kPdone = 1;
    static constexpr size_t vseq_at(size_t ntb) { return kPdone + ntb; }
    static constexpr size_t pread_at(size_t ntb) { return vseq_at(ntb) + ntb * ntb; }
    static constexpr size_t cdone_at(size_t ntb) { return pread_at(ntb) + ntb; }
    static constexpr size_t lead_ticket_at(size_t ntb) { return cdone_at(ntb) + ntb; }
    static constexpr size_t words(size_t ntb) { return lead_ticket_at(ntb) + 1; }
    int *ticket, *pdone, *vseq, *pread, *cdone, *lead_ticket;
    RunCounters(int* base, size_t ntb)
        : ticket(base + kTicket), pdone(base + kPdone), vseq(base + vseq_at(ntb)), pread(base + pread_at(ntb)),
          cdone(base + cdone_at(ntb)), lead_ticket(base + lead_ticket_at(ntb)) {}
};
static_assert(RunCounters::words(1) == 6 && RunCounters::cdone_at(1) == 4, "run counters, ntb = 1");
static_assert(RunCounters::vseq_at(3) == 4 && RunCounters::pread_at(3) == 13 && RunCounters::cdone_at(3) == 16 &&
                  RunCounters::lead_ticket_at(3) == 19 && RunCounters::words(3) == 20,
              "run counters, ntb = 3: 1 + 3 + 9 + 3 + 3 + 1");

// one published tile window: 16 columns of 64 rows of L, then the 16 pivots d
constexpr int kTailPubWin = 16 * 64 + 16;

// The dense-tail sweeps' granules (kkt_sweep.hip gran_put, part_slot) in one
// allocation of words(ntb), sized for 2 right-hand sides: every block's z,
// then from part_at(ntb) on every block's helper partials of k_tail_fwd_lead.
struct ChainGran {
    static constexpr size_t kZ = 2 * 64 * 2;          // per block: right-hand sides x rows x {low, high} half
    static constexpr size_t kPart = 2 * 4 * 64 * 2;   // per block: right-hand sides x column groups x lanes x halves
    static constexpr size_t part_at(size_t ntb) { return ntb * kZ; }
    static constexpr size_t words(size_t ntb) { return ntb * (kZ + kPart); }
};

// (KktPhase, the device-time phases of the KKT core: kkt_schedule.h)
struct KktTimers {
    double phase_ms[kNumPhases] = {};       // accumulated device time per phase
    long phase_launches[kNumPhases] = {};   // kernel launches per phase
    long phase_count[kNumPhases] = {};      // occurrences (factorisations / sweeps)
    double factor_ms = 0.0;   // accumulated device time of factor()
    double solve_ms = 0.0;    // accumulated device time of solve()
    double sweep_ms = 0.0;    // forward + backward substitution sweeps (timing mode)
    long factors = 0, solves = 0, rawsolves = 0;
    long panel_redos = 0;     // factorisations redone without the fused panel kernels
    long redo_where[4] = {0, 0, 0, 0};   // ... by the kernel that bailed (k_panel, k_panel_w sparse / tail, k_panel_s)
    long tail_repairs = 0;    // dense-tail block columns redone in place (look-ahead resumed after them)
    long tail_dep_rounds = 0; // k_tail_dep launches of those repairs
};

// The slots of dScal_, one refinement pass's scalars (doubles).  The first
// pass reads [0, kScMaxbc + 2 R) back, a later one [0, kScReadLater).
constexpr int kScRes = 0;       // [2] the residual of each active system
constexpr int kScEps = 4;       // [2] the sweeps' dropped-column eps per right-hand side (sweep_eps())
constexpr int kScIncons = 6;    // dIncons_'s two ints packed into one double
constexpr int kScReadLater = kScIncons + 1;
constexpr int kScMaxbc = 8;     // [2 * 2] max|fx|, max|fy| per system (the first pass's maxbc)
constexpr int kScCount = kScMaxbc + 4;
// The slots of dFacScal_, finish_pass's read-back.
constexpr int kFsNegMinD = 0;   // -min|d| (a max reduction)
constexpr int kFsNdepMax = 1;   // a sharded solve: kFlagNdep and kFlagBail as doubles,
constexpr int kFsBailMax = 2;   // ... the three of them then maximised over the shards
constexpr int kFsFlags = 3;     // [2] the first three flag words packed as ints
constexpr int kFsCount = kFsFlags + 2;

// The Q block of ldlt.c's K (ldlt.c:253-256, 391-394) on the y-nodes:
// K_yy = -max(E, eps) - qmax Q, Q m x m full symmetric CSC (kkt_plan.h
// QPattern), qmax = the reference's lp->max (-1 max, 1 min).
struct QBlock {
    const int* kQ = nullptr;
    const int* iQ = nullptr;
    const double* Q = nullptr;
    int qmax = 1;
};

struct PlanView;   // kkt_kernels.h

class KktDevice {
  public:
    // A is the solver's m x n matrix (CSC).  The plan (ordering, supernodes)
    // is computed here on the host.  kA/iA/A must outlive nothing: copied.
    // nforced > 0: the last nforced rows (linking rows of a block-angular
    // shard) form the dense tail (kkt_plan.h); with an Exchange set, the
    // tail Schur complement, the tail right-hand sides and the refinement
    // residual of those rows are summed over the shards (exchange.h).
    // qb: an optional Q block (not with nforced > 0).
    KktDevice(int m, int n, const int* kA, const int* iA, const double* A, hipStream_t stream, int nforced = 0,
              const QBlock* qb = nullptr);
    ~KktDevice();
    KktDevice(const KktDevice&) = delete;
    KktDevice& operator=(const KktDevice&) = delete;

    const KktPlan& plan() const { return plan_; }
    void set_exchange(Exchange* x) { xch_ = x; }
    int nforced() const { return nforced_; }
    int m() const { return m_; }
    int n() const { return n_; }
    hipStream_t stream() const { return stream_; }

    // Device copies of the constraint matrix in both orientations.
    const int* kA() const { return dkA_.get(); }
    const int* iA() const { return diA_.get(); }
    const double* A() const { return dA_.get(); }
    const int* kAt() const { return dkAt_.get(); }
    const int* iAt() const { return diAt_.get(); }
    const double* At() const { return dAt_.get(); }
    // Device copy of the Q block (CSC over the m y-nodes); null without entries.
    const int* kQ() const { return qnz_ > 0 ? dkQ_.get() : nullptr; }
    const int* iQ() const { return qnz_ > 0 ? diQ_.get() : nullptr; }
    const double* Q() const { return qnz_ > 0 ? dQ_.get() : nullptr; }
    // The columns of Q with at least knobs_.q_long entries (IPO_HIP_Q_LONG,
    // kkt_knobs.h; any columns, not only trailing ones): their products are
    // summed by one wave each (launch_q_long, dev_common.h) instead of one
    // thread's serial sparse_dot, in the refinement's residual and in
    // IpmSolver::run_qp's.  0 without Q.
    int q_long_count() const { return q_long_n_; }
    int q_long_min() const { return q_long_n_ > 0 ? knobs_.q_long : 0; }   // the kernels' threshold (0: none)
    // out[j] = (Q v)_j for those columns, on the object's stream; the other
    // entries of out (m values) are not written
    void launch_q_long(const double* v, double* out);

    // The forward pre-pass of the next solve's first refinement pass.  That
    // pass's maxbc reduction, its k_perm_in2 and the forward steps [0,
    // h_.sweep.split) (the sparse levels and k_tail_gather) read the sparse
    // panels and the right-hand sides only, both final before the dense tail
    // is factored: given a request, factor() enqueues them on the caller's
    // side stream beside the tail's gather and k_tail_run, ordered by stream
    // events alone, and solve_multi() called next with the same R and vectors
    // starts its first sweep at the tail lead.  The kernels, their arguments
    // and their order are the sequential pass's (bitwise).  Used only when the
    // factorisation's first pass stood with no dependent pivot (the pre-pass
    // ran with eps = 0, ldlt.c:446); otherwise, and at the next factor() or
    // restore_host_state(), it is dropped: the normal pass rewrites all it wrote.
    struct PrePass {
        int R = 0;                        // 1 or 2 right-hand sides
        double* dfy[2] = {nullptr, nullptr};
        double* dfx[2] = {nullptr, nullptr};
        hipStream_t stream = nullptr;     // the side stream (not the object's)
        hipEvent_t ready = nullptr;       // recorded once dfy / dfx hold the right-hand sides
    };
    // New values on the constructor's pattern: dA (its CSC order) and dQ (its
    // kQ / iQ order) are device arrays, validated by the caller (finite, Q
    // symmetric); null: unchanged.  The next factor() and the residual
    // kernels then see what a KktDevice built from those values would.
    void refresh_values(const double* dA, const double* dQ);
    int qnz() const { return qnz_; }
    // Numeric factorisation of K(E, D); E (m), D (n) are device vectors.
    void factor(const double* dE, const double* dD, const PrePass* pre = nullptr);
    // In-place refined solve of  -E dy + A dx = fy,  A' dy + D dx = fx.
    // Returns the rawsolve consistency flag of the last pass (1 = consistent).
    int solve(const double* dE, const double* dD, double* dfy, double* dfx);
    // Two independent refined solves with the same factor (hsd.c:218-224),
    // their substitution sweeps batched; each keeps its own refinement loop.
    int solve2(const double* dE, const double* dD, double* dfy1, double* dfx1, double* dfy2, double* dfx2);
    void solve_multi(int R, const double* dE, const double* dD, double* const* dfy, double* const* dfx, int* ok);

    // One unrefined sweep L D L' z = rhs on R permuted device vectors at dz + r K.
    // (fwd_first: the forward list from that step on, the steps before it done already)
    void rawsolve(double* dz, int R = 1, size_t fwd_first = 0);

    // What a factorisation changes on the host side (eps_diag growth,
    // dependent-pivot count, timers and counters): saved before a
    // speculative factorisation and put back when the caller ends up not
    // using it (the overlapped HSD iteration that finds mu < 1e-12).
    struct HostState {
        double epsdiag;
        int ndep;
        KktTimers tm;
    };
    HostState host_state() const { return {epsdiag_, ndep_, tm_}; }
    void restore_host_state(const HostState& h) { epsdiag_ = h.epsdiag; ndep_ = h.ndep; tm_ = h.tm; drop_prepass(); }

    double epsdiag() const { return epsdiag_; }
    void set_pivot_tolerance(double t) { pivot_tol_ = t; }   // (starts at IPO_HIP_PIVTOL, kkt_knobs.h)
    void set_epsdiag(double e) { epsdiag_ = e; }
    // The refinement's residual takes rows row0..m-1 (trailing long rows, an
    // unsharded solve) from one wave each (launch_link_ax: lanes strided,
    // then a wave sum -- a fixed order, not sparse_dot's) instead of one
    // thread's serial sparse_dot.  For LPs on the segmented-dot policy only
    // (IpmSolver, dev_common.h kOrderedMaxLen).
    void set_long_rows(int row0);
    double pivot_tolerance() const { return pivot_tol_; }
    int ndep() const { return ndep_; }
    int last_passes() const { return last_passes_; }
    const KktTimers& timers() const { return tm_; }
    void enable_timing(bool on) { timing_ = on; }
    void reset_timers() { tm_ = KktTimers(); }

    // Diagnostics: copy numeric factor to host (panels + D), for tests.
    void download_factor(double* lx, double* d, int* live = nullptr) const;
    double* device_lx() const { return dLx_.get(); }
    double* device_diag() const { return dDg_.get(); }

  private:
    const KktKnobs knobs_ = KktKnobs::from_env();   // every runtime knob, read once (kkt_knobs.h)
    // the constructor's steps, in order: each calls its pure function of
    // kkt_schedule.h, uploads the arrays and keeps the host part in h_
    // (what crosses steps is passed; the parts are locals of their step)
    void upload_plan(const int* kA, const int* iA, const double* A, const std::vector<int>& kat,
                     const std::vector<int>& iat, const std::vector<double>& at, const QBlock* qb);
    void build_panel_units();
    SolveChunks build_solve_chunks();
    SweepOrder build_sweep_order(const SolveChunks& ch);
    void build_sync_free_plan(const SolveChunks& ch, const SweepOrder& so, int cus);
    void build_gather_chunks(const VisitSlots& vs);
    void count_work();
    void build_slot_records(const std::vector<int>& kslot_v);
    void setup_tail(int cus);
    void alloc_numeric();
    // (kkt_sweep.hip) the dynamic-LDS limit of the sweep kernels this plan
    // launches: the sync-free ones, or the dense tail's chain, pair and lead kernels
    void raise_sweep_lds(bool sync_free);
    void dump_sf_stamps() const;   // (kkt_sweep.hip) ~KktDevice's developer dump; nothing without -DIPO_SF_STAMPS
    KktLaunch h_;                  // what the launch code reads of the schedule on the host
    PlanView plan_view() const;
    // the host repair backs the look-ahead panel's dependent pivots (TailView::dep):
    // not without the fused kernels, not in a sharded solve
    bool tail_repair() const { return use_panel_ && !xch_ && knobs_.tail_repair; }
    void factor_core(const double* dE, const double* dD, const PrePass* pre);
    void dump_factor(const double* dE, const double* dD, double eps_in);
    int dump_count_ = 0;
    TailView tail_view() const;
    template <int R>
    void sweep(double* dz, const double* epsp, size_t fwd_first);   // rawsolve's sweeps, sf_tbase, tail_rhs_*: kkt_sweep.hip
    // launches one list of h_.sweep in order; returns the kernels it launched
    template <int R>
    int run_sweep_steps(const std::vector<SweepStep>& steps, bool forward, double* dz, const double* epsp,
                        size_t first = 0, size_t last = SIZE_MAX, hipStream_t s = nullptr);   // steps [first, last) on s (null: stream_)
    void tail_rhs_begin(double* dz, int R);
    void tail_rhs_end(double* dz, int R);
    DevBuf<int> dIncons_;          // per right-hand side: inconsistent-system flag
    int launch_gather(const struct PlanView& pv, const TailView& tv, int tail, int group, hipStream_t s);
    void launch_reduce_maxabs2(const double* a, int na, const double* b, int nb, double* dst);

    int m_, n_, T_;
    int nforced_ = 0;
    Exchange* xch_ = nullptr;      // not owned
    DevBuf<double> dLinkAx_;       // [2 * nforced] linking-row products A_link dx per right-hand side
    int long_row0_ = -1;           // set_long_rows: rows >= it by one wave each (-1: none)
    DevBuf<double> dLongAx_;       // [2 * (m - long_row0_)] their products A dx per right-hand side
    bool shard_minor() const { return xch_ && xch_->rank() != 0; }   // holds replicas of the linking rows
    void xsum(double* d, size_t n, RedOp op) { if (xch_) xch_->allreduce(d, n, op, stream_); }
    hipStream_t stream_;
    KktPlan plan_;
    double epsdiag_ = 1.0e-14;     // ldlt.c:31, grows x10 (ldlt.c:301-305)
    int ndep_ = 0;
    // Zero-pivot test |d| <= tol * sum|terms| (the reference tests d == 0,
    // which in its own operation order catches exact cancellations; a
    // different summation order can leave a residue below one ulp of the
    // largest term instead).  1e-17 was chosen by sweeps over the netlib
    // set (a host emulation of the GPU factor in round 1, tools/tau_sweep.py on the GPU):
    // 2^-46 over-flags twin-column pivots the reference keeps, exact zero
    // under-flags; 1e-17 matched the most hsd and intpt iteration counts.
    double pivot_tol_ = knobs_.pivtol;
    int last_passes_ = 0;
    bool timing_ = false;
    KktTimers tm_;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr, ev2_ = nullptr, ev3_ = nullptr;
    std::vector<hipEvent_t> kev_;   // event pool (timing mode)
    size_t kev_used_ = 0;
    struct PhaseMark { hipEvent_t b, e; int phase, launches; };
    std::vector<PhaseMark> marks_;
    hipEvent_t mark_b_ = nullptr;
    hipEvent_t next_event();
    void ph_begin(hipStream_t s);
    void ph_end(int phase, int launches, hipStream_t s);
    void ph_collect();               // after a stream sync
  public:
    // algorithmic flops / bytes of one occurrence of each phase
    double work_flops[kNumPhases] = {}, work_bytes[kNumPhases] = {};
  private:

    // matrix
    DevBuf<int> dkA_, diA_, dkAt_, diAt_;
    DevBuf<double> dA_, dAt_;
    DevBuf<int> dtmap_;            // dAt_[d] = dA_[dtmap_[d]] (value_maps.h csr_value_map)
    DevBuf<int> dqdiagmap_;        // dQdiag_[j] = dQ_[dqdiagmap_[j]], 0 where -1 (q_diag_map)
    // Q block (qnz_ > 0): CSC, its assembly map, its diagonal by y-node (old order)
    int qnz_ = 0, qmax_ = 1;
    DevBuf<int> dkQ_, diQ_;
    DevBuf<double> dQ_, dQdiag_;
    DevBuf<int64_t> dqmap_;
    int q_long_n_ = 0;             // columns of Q summed by one wave each (q_long_count)
    DevBuf<int> dQLongCols_;       // [q_long_n_] those columns, ascending
    DevBuf<double> dLongQ_;        // [2 * m] their products Q dy per right-hand side (full-length vectors)
    // plan
    DevBuf<int> dcol0_, drowptr_, drows_, dperm_, diperm_;
    DevBuf<int64_t> doff_, damap_, ddslot_, drelptr_;
    DevBuf<int> dunit_sup_, dunit_tile_, dtask_ptr_, dtask_pair_, dtask_i0_, dtask_i1_;
    DevBuf<int> dupd_src_, dupd_r0_, dupd_r1_, drel_, dlevel_sups_;
    DevBuf<int> dyrow_ptr_, dyrow_idx_;
    // deep trees: the narrow range's update lists without the values from
    // below the range, and those values' lists for the pre-pass (k_fwd_pre)
    DevBuf<int> dylate_ptr_, dylate_idx_, dpre_col_, dpre_ptr_, dpre_idx_;
    DevBuf<double> dYbuf_;
    // sync-free top levels of the sweeps (k_fwd_sf / k_bwd_sf)
    int sf_grid_ = 1;
    int sf_fwd_epoch_ = 0, sf_bwd_epoch_ = 0;
    long long sf_ticket_next_[2] = {0, 0};   // work-item ticket counters (forward, backward): next launch's base
#ifdef IPO_SF_STAMPS
    std::vector<SchedInt2> h_sf_items_f_;    // forward sync-free items (host copy, developer stamps)
#endif
    int sf_tbase(int d, int nitems, hipStream_t s);
    DevBuf<int2> dsf_items_f_, dsf_items_b_;
    DevBuf<int> dsf_need_, dsf_par_, dsf_zbase_, dsf_zpi_, dsf_fcnt_, dsf_fflag_, dsf_bcnt_, dsf_bflag_, dsf_ticket_;
    DevBuf<int> dybase_;                  // per supernode: first ybuf slot of its update values
    DevBuf<double> dZpad_;                // padded z slices of the range, 2 right-hand sides
    DevBuf<int> dfu_sup_, dfu_j_;         // fused panel unit -> supernode, tile pair index (per level: h_.fu_ptr)
    DevBuf<int> dsmall_sups_;             // small panels (per level: h_.small_ptr)
    const bool use_panel_ = knobs_.panel; // fused diagonal-block + panel kernels
    bool factor_pass(const double* dE, const double* dD, bool fused, bool tail_fused, const PrePass* pre = nullptr);
    // the forward pre-pass (PrePass above; IPO_HIP_PREPASS, kkt_knobs.h)
    bool prepass_eligible(const PrePass* pre, bool fused, bool tail_fused) const;
    void enqueue_prepass(const PrePass& pre);   // the fork after the sparse levels; records ev_pre_done_
    void run_prepass_steps(int R, hipStream_t q);   // (kkt_sweep.hip)
    void enqueue_pass_head(int R, double* const* dfy, double* const* dfx, double* part, hipStream_t s);
    bool take_prepass(int R, double* const* dfy, double* const* dfx);
    void drop_prepass() {
        if (pre_state_ != kPreNone) { pre_state_ = kPreNone; pre_discarded_++; lead_discarded_ += pre_lead_; }
        pre_lead_ = false;
        lead_pending_ = 0;
    }
    enum { kPreNone = 0, kPreEnqueued, kPreValid };
    int pre_state_ = kPreNone;     // Enqueued: inside factor_core, its verdict pending; Valid: the next solve may use it
    PrePass pre_req_;              // the request the enqueued pre-pass ran with
    hipEvent_t ev_pre_fork_ = nullptr, ev_pre_done_ = nullptr;
    long pre_used_ = 0, pre_discarded_ = 0;    // (IPO_HIP_DEBUG_REDO)
    // The pre-pass extended by the forward tail lead in its trailing form
    // (IPO_HIP_LEAD_TRAIL, kkt_knobs.h; k_tail_fwd_lead<R, true>, DESIGN.md
    // 6.6): enqueue_prepass asks for it (lead_pending_: the mode),
    // launch_tail_from(0, true) enqueues it after k_tail_run (pre_lead_), and
    // it stands or is dropped with the pre-pass; the solve then starts its
    // first sweep at h_.sweep.lead_end.
    int lead_pending_ = 0;
    bool pre_lead_ = false;
    hipEvent_t ev_run_reset_ = nullptr;        // mode 2: the run's counters are reset
    long lead_used_ = 0, lead_discarded_ = 0;  // (IPO_HIP_DEBUG_REDO)
    void launch_lead_trail(int R, hipStream_t s, bool beside);   // (kkt_sweep.hip)
    DevBuf<double> dPrePart_;      // the pre-pass's maxbc partials (dPart_ is finish_pass's meanwhile)
    void enqueue_levels(const PlanView& pv, const TailView& tv, bool fused, hipStream_t s, const PrePass* pre);
    bool finish_pass(bool fused);
    void repair_tail();
    DevBuf<int> dsweep_sups_;             // level_sups in sweep order (leaves first on unchunked levels)
    DevBuf<int> dchunk_sup_, dchunk_r0_, dsup_chunk0_;
    DevBuf<double> dPartial_;    // backward partial sums, one 64-vector per chunk
    // split-K gather chunks per group (sparse level l, group nlevels = tail)
    int gst_group_ = knobs_.gather_stamps, gst_n_ = 0;   // developer gather stamps: one launch, then -1
    DevBuf<long long> dGStamp_;
    // (per group: h_.ck_ptr; h_.ck_kind 0 k_update, 1 k_update_flat, 2 k_update_quad; h_.ck_wide k_update<4>)
    DevBuf<int> dck_u_, dck_b_, dck_e_, dck_part_, dsp_u_, dsp_p0_, dsp_n_;
    DevBuf<int> dck_q_;          // split-unit index of each chunk (-1: unsplit)
    DevBuf<int> dSplitCnt_;      // arrival counters of the split units (fused split-K), zero between launches
    bool eps_cleared_ = false;   // solve_multi's k_perm_in has zeroed the sweep's eps slots
    DevBuf<double> dPartialTile_;
    DevBuf<TaskSrc> dusrc_, dtsrc_;   // per gather task: source panel descriptor
    DevBuf<SlotRec> dslot_rec_, dtail_slot_rec_;   // per gather k-slot record (sparse units, dense tail)
    DevBuf<unsigned long long> dChainGran_;   // dense-tail sweep chains: epoch-tagged granules (ChainGran)
    int chain_epoch_ = 0;      // the chains' launch epoch (one per launch, never reused)
    DevBuf<int> dtail_task_ptr_, dtail_kslot_, dtail_kslot_ptr_;
    DevBuf<int> dlead_ticket_;         // k_tail_fwd_lead's role tickets (never reset within a run)
    long long lead_ticket_next_ = 0;
    DevBuf<unsigned> dvisit_list_;     // TailView::vlist (tail_visit_schedule; knobs_.visit_sched off: none)
    // the dense tail as one persistent launch (k_tail_run; knobs_.tail_run off: one launch per step)
    DevBuf<uint2> drun_items_;         // tail_run_schedule (first item of each launch: h_.run_ptr)
    DevBuf<int> drun_cnt_;             // RunCounters
    RunCounters run_counters() const { return RunCounters(drun_cnt_.get(), plan_.ntb); }
    // the run's window hand-off (TailRun::pub; knobs_.tail_winpub)
    DevBuf<double> drun_pub_;          // [2 * ntb * 4 * kTailPubWin]
    DevBuf<int> drun_wflag_;           // [ntb * ntb * 4], zeroed once
    int run_epoch_ = 0;
    // the run of launches [t0, ntb) (reset: a factorisation's first run, counters zeroed)
    void launch_tail_from(int t0, bool reset);
    DevBuf<uint64_t> dtail_tasks_, dutasks_;
    DevBuf<double> dW_;
    DevBuf<double> dDepSt_;        // k_tail_dep's block state and per-tile maxima
    DevBuf<int> dDepI_;            // its round counters
    // numeric
    DevBuf<double> dLx_, dDg_;
    DevBuf<int> dLive_;
    DevBuf<double> dDscale_;
    DevBuf<int> dFlags_;           // PlanView::flags (kFlagWords, kkt_flags.h)
    DevBuf<int> dSign_;            // PlanView::sign
    DevBuf<double> dZ_, dDy_, dDx_, dRy_, dRx_;
    DevBuf<double> dPart_;
    DevBuf<double> dScal_;         // [kScCount] a refinement pass's scalars
    double* sweep_eps() const { return dScal_.get() + kScEps; }
    // finish_pass's read-back has slots of its own ([kFsCount]): the pre-pass's
    // k_perm_in2 zeroes kScEps and its maxbc stands in kScMaxbc while
    // finish_pass runs
    DevBuf<double> dFacScal_;
    double* hScal_ = nullptr;      // pinned: the read-back of dScal_ or dFacScal_
    int* hDepDone_ = nullptr;      // pinned: repair_tail's read-back of k_tail_dep's done word
    FactorVerdict verdict_;        // of the last factor pass (finish_pass)
};

}  // namespace ipo

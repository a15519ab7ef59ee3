// Ros1 time step with X carried as a dense symmetric matrix (driver: gdre.hip; operator products of the shift cycle: adi_cycle.hip).
#include "dense_x.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>

#include "adi_cycle.hpp"
#include "hostla.hpp"
#include "profiling.hpp"

#include "engine_internal.hpp"

namespace dre {

// =============================================================================================
// Ros1 with X carried as a dense symmetric n x n matrix between the time steps (small n).
// At these sizes every compression already forms the n x n matrix L D L' (the factors have more columns than rows: warm start
// + ~17 ADI increments of ~64 columns each), so the factored form buys nothing between two steps: the compression of X after
// every Lyapunov solve (adi.jl:78-80) — a strictly sequential chain of ~9 Householder panels per step that bounded the whole time
// loop — disappears, and the warm-start residual of the step's Lyapunov equation (lyapunov/residual.jl:3-31 applied to
// lowrank_ros1.jl:39-47) collapses to the Riccati residual
//     Res = C'C + K'K + E'XE/tau + F'XE + E'XF = C'C - K'K + A'XE + (A'XE)'          (F = A - E/(2 tau) - B K,  K = B'XE),
// three SpMMs and one fused assembly kernel.  The ADI iteration itself is unchanged (low-rank residual factor, low-rank increments,
// adi.jl:97-179); X_i = X_{i-1} + sum_j (-2 mu_j) V_j T V_j' is one GEMM.  The LDL' form of X is produced once at the end (and by
// the generic path whenever save_state asks for every X(t)).
// =============================================================================================
__global__ __launch_bounds__(256) void k_dense_residual(int n, int q, int m, const double* __restrict__ Ct, int ldc, const double* __restrict__ Kt, int ldk,
                                                        const double* __restrict__ M, int ldm, const double* __restrict__ EY, int ldey, double inv_tau,
                                                        double* __restrict__ Res, int ldres, double* __restrict__ part) {
    __shared__ double red[17];
    const int i = blockIdx.x * 16 + (threadIdx.x & 15), j = blockIdx.y * 16 + (threadIdx.x >> 4);
    double s = 0.0, s2 = 0.0;
    if (i < n && j < n) {
        double cc = 0.0, kk = 0.0;
        for (int l = 0; l < q; ++l) cc += Ct[i + (size_t)l * ldc] * Ct[j + (size_t)l * ldc];
        for (int l = 0; l < m; ++l) kk += Kt[i + (size_t)l * ldk] * Kt[j + (size_t)l * ldk];
        const double mm = M[i + (size_t)j * ldm] + M[j + (size_t)i * ldm];
        const double ey = 0.5 * (EY[i + (size_t)j * ldey] + EY[j + (size_t)i * ldey]);
        const double res = (cc - kk) + mm;
        Res[i + (size_t)j * ldres] = res;
        const double rhs = (cc + kk) + inv_tau * ey;              // right-hand side of the step's Lyapunov equation (lowrank_ros1.jl:42-43)
        s = rhs * rhs;
        s2 = res * res;
    }
    // block_sum (dense.hip) is not visible here: fixed-order reduction through LDS
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    s = wave_sum_d(s);
    s2 = wave_sum_d(s2);
    if (lane == 0) { red[wave] = s; red[4 + wave] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t slot = blockIdx.x + (size_t)gridDim.x * blockIdx.y, ntot = (size_t)gridDim.x * gridDim.y;
        part[slot] = (red[0] + red[1]) + (red[2] + red[3]);
        part[ntot + slot] = (red[4] + red[5]) + (red[6] + red[7]);      // ||Res||_F^2: the first termination norm of the band reduction
    }
}
// control block of the Lyapunov solve: residual = R D R' with orthonormal R, so its norm is ||D||_F
// Workgroup 0: control block of the Lyapunov solve.  Workgroups 1..: the initial residual R (n x J) in the B-operand lane order of the fast
// chain (dense.hpp, AdiFastArgs::Rpc; four 64-entry blocks per workgroup) — rides on this launch instead of a launch of its own.
__global__ __launch_bounds__(256) void k_adi_init_state(int J, const double* __restrict__ D, int ldd, const double* __restrict__ tols, int maxiters, AdiState* st,
                                                        double* __restrict__ nws, int nws_n, int n, int ct, int nblk, const double* __restrict__ R, int ldr,
                                                        double* __restrict__ Rp, const double* __restrict__ warm_tols) {
    if (blockIdx.x > 0) {
        const int blk = (blockIdx.x - 1) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (blk >= nblk) return;
        const int t = blk / ct, j = blk - t * ct;
        const int row = 4 * t + (lane >> 4), col = 16 * j + (lane & 15);
        Rp[(size_t)blk * 64 + lane] = (row < n && col < J) ? R[row + (size_t)col * ldr] : 0.0;
        return;
    }
    __shared__ double red[4];
    for (int i = threadIdx.x; i < nws_n; i += 256) nws[i] = 0.0;        // meeting point of the fast chain's norm workgroups (was a memset of its own)
    double s = 0.0;
    for (int id = threadIdx.x; id < J * J; id += 256) { const double x = D[id % J + (size_t)(id / J) * ldd]; s += x * x; }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double nrm = sqrt((red[0] + red[1]) + (red[2] + red[3]));
        st->iters = 0; st->maxiters = maxiters; st->smw_singular = 0;
        st->abstol = tols[0]; st->res_norm = nrm; st->norms[0] = nrm;
        st->done = (nrm <= tols[0]) ? 1 : 0;
        // warm-started compression (warm.hip): a rejected probe ends the solve before its first iteration — nothing is applied to X, the host
        // redoes the step with the full band reduction
        if (warm_tols && warm_tols[5] != 0.0) st->done = 1;
    }
}

// the context's parked thread number `slot` (created on first use, joined when the context goes)
SideWorker& parked_worker(Ctx* ctx, int slot) {
    if (!ctx->parked_worker[slot]) ctx->parked_worker[slot] = std::shared_ptr<void>(new SideWorker, [](void* p) { delete static_cast<SideWorker*>(p); });
    return *static_cast<SideWorker*>(ctx->parked_worker[slot].get());
}

// the side stream's set-up of the NEXT time step, enqueued by the parked thread as soon as the step's feedback K is on the main stream
// (`job` last: joined before the products it writes go)
struct PreSide { CycleOps co; bool ok = true; GaleOperator op; const double* Kt_p = nullptr; SideWorker::Job job; };

// optional timing of the step's phases: DRE_TRACE=phase (events at the phase boundaries of every step, summed at the end) and
// DRE_TRACE=first (host clock at the phase marks of the FIRST dense step of a run)
struct DenseXTrace {
    bool warm = env_trace("warm"), phase_on = env_trace("phase"), first_on = env_trace("first");
    std::vector<hipEvent_t> pev;
    std::vector<int> ptag;
    std::vector<std::pair<int, std::chrono::steady_clock::time_point>> first_t;
    void mark(Ctx* ctx, int tag, bool first_step) {
        if (first_on && first_step) first_t.push_back({tag, std::chrono::steady_clock::now()});
        if (!phase_on) return;
        hipEvent_t e; (void)hipEventCreate(&e); (void)hipEventRecord(e, ctx->stream);
        pev.push_back(e); ptag.push_back(tag);
    }
    void report() {
        if (first_on && first_t.size() >= 2) {
            std::fprintf(stderr, "[first step, host us]");
            for (size_t i = 1; i < first_t.size(); ++i)
                std::fprintf(stderr, " ->%d %.0f", first_t[i].first, std::chrono::duration<double, std::micro>(first_t[i].second - first_t[i - 1].second).count());
            std::fprintf(stderr, "\n");
            first_t.clear();
        }
        if (!phase_on || pev.size() < 2) return;
        (void)hipEventSynchronize(pev.back());
        static const char* names[] = {"start", "assembly", "band_reduce", "basis+init", "adi_chain", "sync+xupdate", "feedback"};
        double acc[8] = {0};
        for (size_t i = 1; i < pev.size(); ++i) { float ms = 0; (void)hipEventElapsedTime(&ms, pev[i - 1], pev[i]); if (ptag[i] > 0 && ptag[i] < 8) acc[ptag[i]] += ms; }
        double tot = 0; for (int i = 1; i < 7; ++i) tot += acc[i];
        std::fprintf(stderr, "[phase timing, ms per solve] ");
        for (int i = 1; i < 7; ++i) std::fprintf(stderr, "%s %.2f | ", names[i], acc[i]);
        std::fprintf(stderr, "sum %.2f\n", tot);
        for (auto e : pev) (void)hipEventDestroy(e);
        pev.clear(); ptag.clear();
    }
};

struct DenseXState {
    Ctx* ctx = nullptr;
    Mat X;        // n x n, symmetric
    Mat P1;       // E' X
    Mat P1t;      // X E (= P1'), written by the same SpMM launch
    Mat Kt;       // K' = E' X B  (n x m)
    int hint = 0; // ADI iterations of the previous step
    GroupBase gb; // K-independent operator products of the group chain (built at the first dense step)
    // warm-started residual compression (warm.hip): QO[b] = [Om_p (16 Gaussian probe columns) | Q], Q = the orthonormal factor of the last
    // compressed residual (zero padded beyond warm_J); the next factor is written into the other buffer
    Mat QO[2];
    int qcur = -1, q_cols = 0, warm_J = 0, dense_steps = 0;
    // eigenbasis of a cold compression, formed BESIDE the time loop on a helper stream (warm.hip, warm_eig): 0 none, 1 in flight, 2 in use
    int eig_state = 0, eig_k = 0;
    Mat eig_Q, eig_T, eig_U;
    Ctx* eig_hc = nullptr;
    SideWorker* worker = nullptr; // parked host thread that enqueues the side stream's set-up beside the main thread (warm path: the step is bound by host launches)
    double est_ratio = -1.0;      // (probe estimate / tolerance)^2 of the last warm step: what the next truncation may use of the budget
    DevArr<int> tickets;
    long warm_used = 0, warm_rejected = 0;
    DenseXTrace trace;
    // pinned host landing zone: control block, tolerances and the SMW breakdown flag come back with ONE synchronisation per chunk
    struct Landing { AdiState st; double tols[12]; int serr; };
    Landing* land = nullptr;
    // What the parked thread does for this run ACROSS steps (the worker holds one job: at most one of the two is pending).  Declared last: a
    // job reads the members above.
    std::unique_ptr<PreSide> pre;      // the next step's side set-up (side_prefetch)
    SideWorker::Job base_job;          // the group chain's K-independent base (first dense step of a run), joined by the next step
    // (the zone belongs to the context: a pinned allocation and its release cost ~0.1 ms each, per solve)
    DenseXState(Ctx* c, SideWorker* w) : ctx(c), worker(w) {
        if (!ctx->dense_land && hipHostMalloc(&ctx->dense_land, 16384, hipHostMallocDefault) != hipSuccess) ctx->dense_land = nullptr;
        static_assert(sizeof(Landing) <= 16384, "landing zone");
        land = (Landing*)ctx->dense_land;
    }
    // The parked threads outlive the solve (they live with the context); a job still running when the run ends — on the regular exit of a
    // one-step run or on an exception — would go on reading this state, the options and the factor cache of a dead frame (found by the
    // option matrix: a heap corruption that surfaced in the NEXT numpy call of a one-step test).
    ~DenseXState() {
        const bool pending = base_job.pending() || (pre && pre->job.pending());
        base_job.reset();
        if (pre) pre->job.reset();
        if (pending && ctx->side) (void)hipStreamSynchronize(ctx->side->stream);          // (what the job enqueued reads buffers of this run)
        if (eig_state == 1 && eig_hc) (void)hipStreamSynchronize(eig_hc->stream);         // (its buffers go back to the pool behind it)
    }
    DenseXState(const DenseXState&) = delete;
    DenseXState& operator=(const DenseXState&) = delete;
};
// SMW products and the (group) stacks of a time step on the side stream: they depend on K only.  Records ctx->side_e2 behind them.
static void dense_group_base(Ctx* ctx, Ctx* wctx, DenseXState& sx, const GaleOperator& op, const AdiOptions& adi, const CycleOps& co, int n, int m) {
    (void)ctx; (void)n; (void)m;
    // first dense step of a run: the K-independent operator products (8 GEMMs + ~30 small launches per run) are formed on the side
    // stream BEHIND the event the chain waits for — this step runs the one-iteration chain, the group chain takes over from the next
    const int gwant = group_size_for(ctx, (int)adi.shifts.values.size(), n, m);
    bool distinct = true;                       // (a cycle with repeated values keeps the single-iteration chain)
    for (size_t i = 0; i < adi.shifts.values.size(); ++i)
        for (size_t j = 0; j < i; ++j) distinct = distinct && adi.shifts.values[i].real() != adi.shifts.values[j].real();
    if (distinct) group_base_build(wctx, op, adi.shifts.values, co, sx.gb, gwant);
}
// want_base (optional): the K-independent base of the group chain is NOT built here; *want_base tells the caller to do it (dense_group_base)
static void dense_side_setup(Ctx* ctx, Ctx* wctx, DenseXState& sx, const GaleOperator& op, const AdiOptions& adi, FactorCache* cache, int n, int m, CycleOps& co,
                             bool& co_ok, bool* want_base = nullptr) {
    if (wctx != ctx) DRE_HIP(hipStreamWaitEvent(wctx->stream, ctx->side_e1, 0));
    // group chain: the K-independent operator products are built at the first dense step of a run; from then on the SMW products of
    // every step land in the persistent buffers the left-factor descriptors point into
    const int gwant = group_size_for(ctx, (int)adi.shifts.values.size(), n, m);       // (the MAIN context's options)
    bool gb_ok = gwant >= 2 && (int)adi.shifts.values.size() / gwant <= 8 && sx.gb.g == gwant && sx.gb.tag == op.tag && sx.gb.m == m &&
                 sx.gb.mus.size() == adi.shifts.values.size();
    for (size_t i = 0; gb_ok && i < sx.gb.mus.size(); ++i) gb_ok = sx.gb.mus[i] == adi.shifts.values[i].real();
    co_ok = cycle_ops_prepare(wctx, op, adi.shifts.values, cache, co, gb_ok ? &sx.gb.wks : nullptr, gb_ok ? &sx.gb.spack : nullptr, gb_ok);
    if (co_ok && gb_ok) group_ops_prepare(wctx, adi.shifts.values, co, sx.gb);
    const bool build_group_base = co_ok && !gb_ok && gwant >= 2 && (int)adi.shifts.values.size() / gwant <= 8;
    if (wctx != ctx) DRE_HIP(hipEventRecord(ctx->side_e2, wctx->stream));
    if (want_base) *want_base = build_group_base;
    else if (build_group_base) dense_group_base(ctx, wctx, sx, op, adi, co, n, m);
}

// ---- one Ros1 step on the dense state -------------------------------------------------------------------------------------------------
constexpr int WARM_QCAP = 64;       // widest basis (warm.hip: q + 16 <= 80)

// The side stream's share of a step — the SMW products and the folded stacks, which depend on K only — and the ONE owner of the hand-shake
// with the parked thread: whether the set-up is the one the previous step prefetched, is enqueued by this thread (run) or by the parked
// thread beside this one (start), where it is joined (join: `co` and `co_ok` are valid behind it), the hand-over of the group chain's base
// to the parked thread and the prefetch for the next step (finish).  The main stream waits for the set-up through ctx->side_e2.
// Leaving the step early (refusal or exception) after the side stream was set up: the caller falls back to the generic ADI on the MAIN stream
// with the same factor cache, whose entries (stacks, dense inverses, SMW products) and op.Vt the side stream may still be touching — the
// destructor joins the job and both streams on the host before anything of the step's frame is released or reused.
class SideSetup {
  public:
    SideSetup(Ctx* ctx, Ctx* wctx, DenseXState& sx, const GaleOperator& op, const AdiOptions& adi, FactorCache* cache, int n, int m, bool more_steps, CycleOps& co,
              bool& co_ok)
        : ctx(ctx), wctx(wctx), sx(sx), op(op), adi(adi), cache(cache), n(n), m(m), more_steps(more_steps), co(co), co_ok(co_ok) {}
    SideSetup(const SideSetup&) = delete;
    SideSetup& operator=(const SideSetup&) = delete;
    ~SideSetup() {
        if (!armed) return;
        job.reset();
        sx.base_job.reset();
        if (wctx != ctx) (void)hipStreamSynchronize(wctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
    }
    // top of the step: the group base of the previous step is through; is this step's set-up under way already?
    void begin() {
        sx.base_job.wait();
        if (sx.pre && sx.pre->job.pending()) {
            // the parked thread is enqueueing (or has enqueued) this step's side-stream work since the end of the previous step: it is joined
            // where `co` is needed, in front of the chain — not here, so that the two threads enqueue their streams side by side
            if (sx.pre->op.tag == op.tag && sx.pre->Kt_p == (const double*)sx.Kt.p) { job = std::move(sx.pre->job); prefetched = ran = armed = true; }
            else {          // (another operator: e.g. a change of the step size) — drop it
                try { sx.pre->job.wait(); } catch (...) { (void)hipStreamSynchronize(wctx->stream); sx.pre.reset(); throw; }
                DRE_HIP(hipStreamSynchronize(wctx->stream));
                sx.pre.reset();
            }
        }
        if (!prefetched && wctx != ctx) DRE_HIP(hipEventRecord(ctx->side_e1, ctx->stream));          // K of the previous step is ready here
    }
    // enqueued by this thread (unless it ran or runs already)
    void run() {
        if (ran) return;
        ran = armed = true;
        dense_side_setup(ctx, wctx, sx, op, adi, cache, n, m, co, co_ok);
    }
    // the same, handed to the parked worker thread: the main thread goes on enqueueing its own stream and joins before it needs `co`
    // (on ONE context the set-up's own read-backs would nest inside the reduction's: it runs first then)
    void start() {
        if (ran) return;
        if (!sx.worker || wctx == ctx) { run(); return; }
        ran = armed = true;
        const int dev = ctx->device;
        job = sx.worker->submit([this, dev]() { DRE_HIP(hipSetDevice(dev)); dense_side_setup(ctx, wctx, sx, op, adi, cache, n, m, co, co_ok, &want_base); });
    }
    void join() {
        if (!job.pending()) return;
        if (prefetched) {          // the prefetched set-up: take its products over
            try { job.wait(); } catch (...) { sx.pre.reset(); throw; }
            co = std::move(sx.pre->co); co_ok = sx.pre->ok;
            sx.pre.reset();
        } else job.wait();
        if (want_base && !more_steps) want_base = false;          // (the last step of a run: nobody would use the base — nor join the job that builds it)
        if (want_base) {
            // the base of the group chain (~250 launches on the side stream, once per run) is enqueued by the parked thread while this one goes
            // on with the chain; the next step joins it.  (It reads the cycle's factors and stacks: shared with `co` through reference counts.)
            want_base = false;
            auto cop = std::make_shared<CycleOps>(co);
            const GaleOperator opc = op;
            Ctx* const c = ctx; Ctx* const wc = wctx;
            DenseXState* const sxp = &sx;
            const AdiOptions* const adip = &adi;
            const int nn = n, mm = m, dev = ctx->device;
            sx.base_job = sx.worker->submit([c, wc, sxp, opc, adip, cop, nn, mm, dev]() { DRE_HIP(hipSetDevice(dev)); dense_group_base(c, wc, *sxp, opc, *adip, *cop, nn, mm); });
        }
    }
    // regular end of the step (the main stream waited for side_e2: nothing of the side stream is pending); arms the next step's prefetch
    void finish(const GaleOperator& op_base) {
        armed = false;
        if (!(more_steps && sx.worker && wctx != ctx && ctx->side_prefetch != 0)) return;
        // the next step's SMW products and stacks depend on this K only: the parked thread enqueues them NOW (behind an event on the main stream),
        // so that they are finished when the next step's compression is — the side stream's 100 us no longer start after the host has enqueued
        // the next step's main-stream kernels
        sx.base_job.wait();       // (the worker holds ONE job: the group base of the first step must be through)
        DRE_HIP(hipEventRecord(ctx->side_e1, ctx->stream));
        sx.pre = std::make_unique<PreSide>();
        PreSide* const pp = sx.pre.get();
        pp->op = op_base; pp->op.Vt = sx.Kt; pp->Kt_p = (const double*)sx.Kt.p;
        Ctx* const c = ctx; Ctx* const wc = wctx;
        DenseXState* const sxp = &sx;
        const AdiOptions* const adip = &adi;
        FactorCache* const cachep = cache;
        const int nn = n, mm = m, dev = ctx->device;
        pp->job = sx.worker->submit([c, wc, sxp, pp, adip, cachep, nn, mm, dev]() {
            DRE_HIP(hipSetDevice(dev));
            dense_side_setup(c, wc, *sxp, pp->op, *adip, cachep, nn, mm, pp->co, pp->ok);
        });
    }
  private:
    Ctx* const ctx; Ctx* const wctx;
    DenseXState& sx;
    const GaleOperator& op;
    const AdiOptions& adi;
    FactorCache* const cache;
    const int n, m;
    const bool more_steps;
    CycleOps& co;
    bool& co_ok;
    bool prefetched = false, ran = false, armed = false, want_base = false;
    SideWorker::Job job;        // this step's set-up on the parked thread (the prefetched one: taken over from sx.pre)
};

// what a compression of the step's residual hands to the chain:  Res ~ R Tm R'  with orthonormal R (n x k)
struct Compressed {
    int rc = 0;                   // 0 = go on, 1 = the warm-started compression gave up (nothing applied to X: redo the step cold), 2 = the fast chain refuses
    Mat R, Tm;
    int k = 0;
    const double* warm_tols = nullptr;
    int wnext = -1, wq_next = 0;  // buffer of sx.QO that holds this attempt's factor, its columns
};
// the ADI chain of one attempt: the state block's companions and where the host stands
struct Chain {
    DevArr<double> nws, Rp0;      // meeting point of the norm workgroups; the initial residual in the fast chain's B-operand order (slot 0 of the first chunk)
    Mat Gm;
    bool use_pk = false, grp = false, specx = false, any_plain = false, finished = false;
    size_t rpd = 0, cyc = 0;
    int nstrip = 0, kst = 0, gsz = 0, iters_host = 0, vcols_used = 0;
};
struct Chunk { int base_it = 0, nit = 0; size_t cyc0 = 0; Mat Rring; };

// The frame of one step: what the phases share.  The parked thread reads op, adi, cache, co and co_ok through `side` by reference: the frame
// outlives the join (side is declared last: destroyed, and so joined, first) and is never copied or moved.
struct DenseStep {
    CycleOps co;
    bool co_ok = true;
    Ctx* const ctx;
    const GdreProblem& prob;
    const double tau;
    const AdiOptions& adi;
    FactorCache* const cache;
    DenseXState& sx;
    AdiResult& ar;
    const Pencil& P;
    const int n, q, m, nt;
    GaleOperator op;              // the step's operator: its low-rank part carries this step's K
    // SMW products and the folded stacks depend on K only: they are built on the side stream while the main stream assembles and
    // compresses the residual; the ADI chain waits for them through an event
    Ctx* const wctx;
    Mat Mx, EY, Res;
    DevArr<double> part, tols;
    double reltol = 0.0;
    DevArr<AdiState> st;
    AdiState h;
    std::vector<Mat> keepV;
    std::vector<BufP> keepRpk;
    double init_norm = 0.0;
    Mat Vall, Wall;
    int acc_total = 0, k = 0;
    std::vector<double> coef;
    SideSetup side;

    DenseStep(Ctx* ctx, const GdreProblem& prob, const GaleOperator& op_base, double tau, const AdiOptions& adi, FactorCache* cache, DenseXState& sx, AdiResult& ar,
              bool more_steps)
        : ctx(ctx), prob(prob), tau(tau), adi(adi), cache(cache), sx(sx), ar(ar), P(*prob.P), n(P.n), q(prob.Ct.cols), m(prob.B.cols), nt(ceil_div(n, 16)), op(op_base),
          wctx((ctx->side && ctx->x_side_stream) ? ctx->side.get() : ctx), side(ctx, wctx, sx, op, adi, cache, n, m, more_steps, co, co_ok) {
        op.Vt = sx.Kt;
    }
    DenseStep(const DenseStep&) = delete;
    DenseStep& operator=(const DenseStep&) = delete;

    void mark(int tag) { sx.trace.mark(ctx, tag, sx.dense_steps == 0); }
    void assemble_residual();
    void adopt_eigenbasis();
    bool warm_try() const;
    Compressed compress_warm();
    Compressed compress_cold();
    void start_eigenbasis(const Compressed& cz);
    int attempt(bool use_warm);
    int run_chain(Compressed& cz, bool use_warm);
    void chain_setup(const Compressed& cz, Chain& c);
    void enqueue_group_chunk(const Compressed& cz, Chain& c, const Chunk& ck);
    void enqueue_single_chunk(const Compressed& cz, Chain& c, const Chunk& ck);
    bool fetch_chunk(Compressed& cz, Chain& c, const Chunk& ck, bool use_warm);
    void late_x_update(const Compressed& cz);
    void next_basis(const Compressed& cz, bool use_warm);
    void close();
};

// Riccati residual at X (= warm-start residual of the step's Lyapunov equation) and the norm of the equation's right-hand side.
// The main stream's kernels are enqueued BEFORE the side stream is set up: the host calls for the side stream (event wait, six
// launches) would otherwise sit in front of them while the main stream idles.
// (Enqueueing the side stream's work before the assembly instead of inside the band reduction's first read-back was measured at n = 371 with
// the group chain: 21.7 against 21.2 ms per solve — the host calls delay the main stream's first kernels by more than the earlier start gains.)
void DenseStep::assemble_residual() {
    Mx = Mat(ctx, n, n); EY = Mat(ctx, n, n); Res = Mat(ctx, n, n);
    const Mat& Y = sx.P1t;                                                      // Y = X E
    spmm_dual(ctx, P, P.valAt.p, P.valEt.p, Y, Mx, EY);       // A' X E and E' X E in one pass over X E
    part = DevArr<double>(ctx, (size_t)2 * nt * nt); tols = DevArr<double>(ctx, 12);
    hipLaunchKernelGGL(k_dense_residual, dim3(nt, nt), dim3(256), 0, ctx->stream, n, q, m, (const double*)prob.Ct.p, prob.Ct.ld, (const double*)sx.Kt.p, sx.Kt.ld,
                       (const double*)Mx.p, Mx.ld, (const double*)EY.p, EY.ld, 1.0 / tau, Res.p, Res.ld, part.p);
    reltol = adi.reltol >= 0 ? adi.reltol : n * EPS;
    mark(1);
}

// Warm-started compression (warm.hip): Rayleigh-Ritz in the basis of the previous step's residual factor, accepted by a 16-column probe.
// Tried from the third dense step of a run on (the second step's residual is several times wider than the first's); a rejected
// attempt is redone with the full band reduction.
void DenseStep::adopt_eigenbasis() {
    if (!(sx.eig_state == 1 && hipEventQuery(aux_event(ctx, 3)) == hipSuccess)) return;
    // the eigenbasis of an earlier cold step's factor is ready (a few steps old by now: the range moves slowly, and the 16 fresh directions
    // of every warm step pick up what it misses)
    sx.eig_state = 2;
    // (its 32 leading directions: the eigenvalues fall off quickly, and the small eigenproblem of the first warm step costs O(m) dependent rounds)
    sx.qcur = 1; sx.q_cols = std::min(sx.eig_k, 32); sx.warm_J = sx.q_cols; sx.est_ratio = -1.0;
    sx.eig_Q = Mat(); sx.eig_T = Mat(); sx.eig_U = Mat();
}
bool DenseStep::warm_try() const {
    return ctx->dense_warm != 0 && sx.eig_state == 2 && sx.qcur >= 0 && sx.q_cols >= 16 && sx.q_cols <= WARM_QCAP && sx.dense_steps >= 2 && n >= 96 && n <= 1024 &&
           sx.q_cols + 32 <= n && !(ctx->dense_x_max_k > 0 && sx.q_cols > ctx->dense_x_max_k);
}

// B = [Q, Z]: the previous step's eigenbasis + 16 fresh directions; the launches are warm.hip's (warm_chain_jacobi: eight; the wide-basis
// variant shares the first five, warm_chain_front)
Compressed DenseStep::compress_warm() {
    Compressed cz;
    const int qb = sx.q_cols, mb = qb + 16;
    const int kl = std::min(qb, std::max(16, ((sx.warm_J + 15) / 16) * 16));       // the chain's width: the previous rank, rounded up
    const int qn = std::min(std::min(mb, WARM_QCAP), kl + (ctx->dense_warm == 2 ? 16 : 0));      // columns of the next basis (the leading eigen-directions; dense_warm = 2: 16 spare ones)
    Mat& QOc = sx.QO[sx.qcur];
    Mat& QOn = sx.QO[1 - sx.qcur];
    WarmChain w;
    w.n = n; w.qb = qb; w.kl = kl; w.qn = qn;
    w.YB = Mat(ctx, n, 64 + qb); w.Z1 = Mat(ctx, n, 16); w.Cc = Mat(ctx, mb, 64 + qb); w.Uc = Mat(ctx, mb, qn); w.Cp = Mat(ctx, mb, 16);
    DevArr<double> slab(ctx, (size_t)nt * 256 + nt + 256);
    w.Pf = Mat(ctx, qb, 16);
    w.Res = Res; w.QOc = QOc; w.QOn = QOn; w.slab = slab.p; w.tickets = sx.tickets.p; w.tols = tols.p;
    w.parts = part.p; w.nparts = nt * nt; w.reltol = reltol; w.abstol = adi.abstol; w.frac = adi.residual_abs_frac;
    w.bf = sx.est_ratio < 0.0 ? 0.4 : std::min(0.6, std::max(0.05, 1.0 - 2.6 * sx.est_ratio));
    side.start();      // (the side stream's dozen launches are enqueued by the parked thread while this one enqueues the compression)
    if (mb <= 48 || ctx->dense_warm != 3) {
        w.Tm = cz.Tm = Mat(ctx, kl, kl);
        warm_chain_jacobi(ctx, w);                      // the eight launches of the Jacobi form (warm.hip)
        Mat Rfull = QOn.colsview(32, qn);
        cz.R = Rfull.colsview(0, kl);
        cz.k = kl;
        cz.wq_next = qn;
    } else {
        // wide basis (the first warm steps behind a cold one: its Krylov basis is not an eigenbasis, and a Jacobi iteration on 80 x 80 from
        // scratch costs a millisecond): the small kernel stops behind the whitening and hands M over; its band reduction (the cold path's
        // kernels on an 80-row matrix, with their read-back) gives a basis of J_b columns, narrow enough for the Jacobi form from the next step on
        warm_chain_front(ctx, w);
        Mat Mw(ctx, mb, mb), LT(ctx, mb, mb);
        cz.Tm = Mat(ctx, kl, kl);
        warm_small(ctx, qb, mb, kl, qn, w.Cc, w.parts, w.nparts, w.reltol, w.abstol, w.frac, w.bf, tols.p, w.Uc, cz.Tm, w.Cp, sx.tickets.p + 1, &Mw, &LT);
        side.join();
        SymBand wsb = sym_band_reduce(ctx, Mw, adi.compress_tolfac, -1.0, tols.p + 3);
        cz.k = wsb.J;
        if (cz.k <= 0 || cz.k > WARM_QCAP) { cz.rc = 1; return cz; }
        Mat Bq = sym_band_basis(ctx, wsb);             // mb x k
        Mat Ub(ctx, mb, cz.k);
        gemm_thin(ctx, false, mb, cz.k, mb, 1.0, LT.p, LT.ld, Bq.p, Bq.ld, 0.0, Ub.p, Ub.ld, nullptr, "warm_project");
        cz.Tm = wsb.D;
        warm_ctl(ctx, tols.p, sx.tickets.p + 1, cz.k);
        Mat Bb = QOc.colsview(32, mb), Yp = w.YB.colsview(0, 16), Rfull = QOn.colsview(32, cz.k);
        warm_finish(ctx, n, mb, cz.k, Bb, Ub, Yp, w.Cp, Rfull, slab.p + (size_t)nt * 256, sx.tickets.p + 1, tols.p);
        cz.R = Rfull;
        cz.wq_next = cz.k;
        keepV.push_back(Mw); keepV.push_back(LT); keepV.push_back(Bq); keepV.push_back(Ub);
    }
    keepV.push_back(w.YB); keepV.push_back(w.Pf); keepV.push_back(w.Z1); keepV.push_back(w.Cc); keepV.push_back(w.Uc); keepV.push_back(w.Cp);
    keepRpk.push_back(slab.buf);
    cz.warm_tols = tols.p;
    cz.wnext = 1 - sx.qcur;
    side.join();
    return cz;
}

// residual factor: Res ~ Q D Q' (band reduction, truncated at a fraction of abstol like the warm-start residual of the generic path)
Compressed DenseStep::compress_cold() {
    Compressed cz;
    BandSpec spec;
    // tols[0] = abstol = reltol ||C_rhs||_F (adi.jl:61-62), tols[1] = truncation tolerance of the residual compression, tols[2] = ||C_rhs||_F:
    // computed by the reduction's control-block launch
    spec.tol_parts = part.p; spec.tol_nparts = nt * nt; spec.tol_reltol = reltol; spec.tol_abstol = adi.abstol; spec.tol_frac = adi.residual_abs_frac;
    spec.tols_out = tols.p;
    side.start();        // (joined behind the reduction: the parked thread enqueues the side stream while this one enqueues the panels)
    SymBand sb = sym_band_reduce(ctx, Res, adi.compress_tolfac, -1.0, tols.p + 1, &spec, part.p + (size_t)nt * nt, nt * nt);
    side.run();
    side.join();
    cz.k = sb.J;
    if (cz.k > 0) {
        cz.R = spec.hit ? spec.B : sym_band_basis(ctx, sb);        // predicted rank: the basis was enqueued during the read-back
        cz.Tm = sb.D;
        start_eigenbasis(cz);
    }
    return cz;
}
// Turn a cold factor into an EIGENBASIS beside the time loop: a Jacobi iteration on T (k x k, a band matrix in Krylov order) takes about a
// millisecond in one workgroup — on a helper stream it costs the time loop nothing, and the warm-started compression (warm.hip) that
// takes over when it is done starts from a nearly diagonal matrix.  Q and T are snapshots: the next cold steps reuse their buffers.
void DenseStep::start_eigenbasis(const Compressed& cz) {
    const int k = cz.k;
    if (!(ctx->dense_warm != 0 && sx.eig_state != 1 && k >= 16 && k <= WARM_QCAP && k + 32 <= n && n >= 96 && n <= 1024 && sx.dense_steps >= 1)) return;
    if (sx.QO[0].empty()) {
        for (int b = 0; b < 2; ++b) { sx.QO[b] = Mat(ctx, n, 32 + WARM_QCAP + 16); Mat om = sx.QO[b].colsview(0, 32); fill_gauss(ctx, om, 0x7F4A7C159E3779B9ull); }
        sx.tickets = DevArr<int>(ctx, 4);
        DRE_HIP(hipMemsetAsync(sx.tickets.p, 0, 4 * sizeof(int), ctx->stream));
    }
    Ctx* const hc = helper_ctx(ctx, 0);
    sx.eig_hc = hc;
    sx.eig_Q = Mat(ctx, n, k); sx.eig_T = cz.Tm; sx.eig_U = Mat(ctx, k, k); sx.eig_k = k;
    copy_mat(ctx, cz.R, sx.eig_Q);
    DRE_HIP(hipEventRecord(aux_event(ctx, 2), ctx->stream));
    DRE_HIP(hipStreamWaitEvent(hc->stream, aux_event(ctx, 2), 0));
    warm_eig(hc, k, sx.eig_T, sx.eig_U);
    Mat dst = sx.QO[1].colsview(32, k);
    gemm_thin(hc, false, n, k, k, 1.0, sx.eig_Q.p, sx.eig_Q.ld, sx.eig_U.p, sx.eig_U.ld, 0.0, dst.p, dst.ld, nullptr, "warm_project");
    DRE_HIP(hipEventRecord(aux_event(ctx, 3), hc->stream));
    sx.eig_state = 1;
}

// one attempt at the step: 0 = done, 1 = the warm-started compression was rejected (nothing applied to X), 2 = the fast chain refuses
int DenseStep::attempt(const bool use_warm) {
    std::memset(&h, 0, sizeof(int) * 4 + sizeof(double) * 3);
    ar = AdiResult();
    keepV.clear(); keepRpk.clear(); coef.clear();
    init_norm = 0.0; acc_total = 0;
    Compressed cz = use_warm ? compress_warm() : compress_cold();
    k = cz.k;
    if (cz.rc != 0) return cz.rc;
    if (!co_ok) return 2;
    mark(2);
    ar.rhs_cols = k;
    if (k > ADI_FAST_MAX_K || (ctx->dense_x_max_k > 0 && k > ctx->dense_x_max_k)) return 2;
    if (k > 0) {
        const int rc = run_chain(cz, use_warm);
        if (rc != 0) return rc;
    } else {
        // zero residual: read the tolerances back for the record
        DRE_HIP(hipMemcpyAsync(sx.land->tols, tols.p, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        DRE_HIP(hipStreamSynchronize(ctx->stream));
        if (wctx != ctx) DRE_HIP(hipStreamWaitEvent(ctx->stream, ctx->side_e2, 0));
    }
    next_basis(cz, use_warm);
    return 0;
}

// control block, packed initial residual, the wait for the side stream, and how the solve is cut into chunks
void DenseStep::chain_setup(const Compressed& cz, Chain& c) {
    c.nws = DevArr<double>(ctx, ADI_FAST_NWS);
    int mode0 = 0, nt0 = 0;
    adi_fast_pick(n, k, &mode0, &nt0);
    c.use_pk = mode0 == 0;
    c.rpd = adi_fast_rpack_doubles(n, k);
    c.Rp0 = DevArr<double>(ctx, c.use_pk ? c.rpd : 1);
    const int pk_ct = (k + 15) / 16, pk_nblk = c.use_pk ? 4 * adi_fast_nstrip(n) * pk_ct : 0;
    hipLaunchKernelGGL(k_adi_init_state, dim3(1 + (pk_nblk + 3) / 4), dim3(256), 0, ctx->stream, k, (const double*)cz.Tm.p, cz.Tm.ld, (const double*)tols.p, adi.maxiters, st.p, c.nws.p,
                       ADI_FAST_NWS, n, pk_ct, pk_nblk, (const double*)cz.R.p, cz.R.ld, c.Rp0.p, cz.warm_tols);
    if (wctx != ctx) DRE_HIP(hipStreamWaitEvent(ctx->stream, ctx->side_e2, 0));
    mark(3);
    c.nstrip = adi_fast_nstrip(n); c.kst = adi_fast_kst(n);
    c.Gm = Mat(ctx, k * k, 2);
    // the whole solve is enqueued at once (one more iteration than the previous step needed); further chunks only if that was not enough
    const int cap = std::max(1, adi.maxiters);
    const int ctk = (k + 15) / 16;
    c.gsz = co.group_g;
    c.grp = c.gsz >= 2 && c.use_pk && k <= ADI_GROUP_MAX_K && c.gsz * ctk * ((ctk + 3) / 4) <= ADI_FAST_NWS - 1 && !co.gpack.empty();
    Vall = Mat(ctx, n, k * (std::min(cap, std::max(adi.compression_interval, sx.hint + 1) + 64) + (c.grp ? c.gsz : 0)));
    // specx: every chunk's update of X is enqueued during its read-back (the batched product takes its descriptors as kernel arguments,
    // 48 at most; chunks never grow within a solve)
    c.specx = std::min(std::max(adi.compression_interval, sx.hint + 1), adi.maxiters) + (c.grp ? c.gsz : 0) <= 48;
}

int DenseStep::run_chain(Compressed& cz, const bool use_warm) {
    Chain c;
    chain_setup(cz, c);
    while (!c.finished) {
        Chunk ck;
        ck.base_it = c.iters_host;
        ck.cyc0 = c.cyc;
        int nit = std::min(std::max(adi.compression_interval, sx.hint + 1), adi.maxiters - c.iters_host);
        nit = std::min(std::min(nit, 480), (Vall.cols - c.vcols_used) / k);        // (< 512: the device keeps the norm history as a ring)
        if (nit <= 0) break;
        // group chain (first chunk of a solve: it starts at position 0 of the cycle): whole groups of gsz iterations per launch; the
        // iteration count of the previous time step (counts fall from step to step) rounded up to a multiple of gsz is enqueued
        const bool grp_now = c.grp && ck.base_it == 0 && c.cyc == 0;
        if (grp_now) {
            const int want = std::min(std::min(std::max(sx.hint, 1), adi.maxiters), 480);
            nit = ((want + c.gsz - 1) / c.gsz) * c.gsz;
            nit = std::min(nit, ((Vall.cols - c.vcols_used) / k / c.gsz) * c.gsz);
        }
        ck.nit = nit;
        ck.Rring = Mat(ctx, n, k * nit);
        keepV.push_back(ck.Rring);
        if (grp_now && nit >= c.gsz) enqueue_group_chunk(cz, c, ck);
        else enqueue_single_chunk(cz, c, ck);
        if (!fetch_chunk(cz, c, ck, use_warm)) return 1;
    }
    acc_total = c.iters_host;
    for (auto& f : co.fe) if (!f->checked) { f->growth = mf_check(ctx, f->f); f->checked = true; }
    if (sx.land->serr) throw Error(ERR_SINGULAR, "SMW: capacitance matrix is singular");
    if (acc_total > 0 && c.any_plain) late_x_update(cz);
    return 0;
}

void DenseStep::enqueue_group_chunk(const Compressed& cz, Chain& c, const Chunk& ck) {
    const int nit = ck.nit, gsz = c.gsz, base_it = ck.base_it;
    const size_t rpd = c.rpd;
    const Mat& Rring = ck.Rring;
    const int NG = nit / gsz, ncyc = (int)adi.shifts.values.size();
    DevArr<double> Rpk(ctx, rpd * (size_t)(nit + 1));
    Mat Gg(ctx, k * k, 2 * gsz);
    AdiGroupArgs ga;
    std::memset(&ga, 0, sizeof(ga));
    ga.n = n; ga.k = k; ga.nstrip = c.nstrip; ga.kst = c.kst; ga.g = gsz;
    ga.ldr = Rring.ld; ga.rpd = rpd; ga.ldv = Vall.ld;
    ga.T = cz.Tm.p; ga.ldt = cz.Tm.ld; ga.alpha = 1.0; ga.st = st.p; ga.nws = c.nws.p;
    double by1 = 0.0, fl1 = 0.0;
    ga.do_strips = 1; ga.n_prev = gsz;
    adi_group_cost(ga, &by1, &fl1);
    {
        TimedScope chain_ts(ctx, "adi_group_iter", by1 * NG, fl1 * NG, NG + 2);
        for (int L = 0; L <= NG + 1; ++L) {
            ga.do_strips = L < NG ? 1 : 0;
            if (L < NG) {
                ga.Gpack = co.gpack[(size_t)(((L * gsz) % ncyc) / gsz)];
                ga.Rpc = L == 0 ? c.Rp0.p : Rpk.p + (size_t)(L * gsz) * rpd;
                ga.Rring = Rring.p + (size_t)(L * gsz) * k * Rring.ld;
                ga.Rpk = Rpk.p + (size_t)(L * gsz + 1) * rpd;
                ga.V = Vall.p + (size_t)(c.vcols_used + L * gsz * k) * Vall.ld;
            }
            // Gram matrices of the residuals launch L - 1 produced; norms + decisions for those of launch L - 2
            ga.n_prev = (L >= 1 && L <= NG) ? gsz : 0;
            ga.Rp_prev = ga.n_prev ? Rpk.p + (size_t)((L - 1) * gsz + 1) * rpd : nullptr;
            ga.G_prev = Gg.p + (size_t)(L & 1) * gsz * k * k;
            ga.n_prev2 = L >= 2 ? gsz : 0;
            ga.G_prev2 = Gg.p + (size_t)((L - 1) & 1) * gsz * k * k;
            ga.it0_prev2 = base_it + (L - 2) * gsz + 1;
            adi_group_iter(ctx, ga);
        }
    }
    for (int j = 0; j < nit; ++j) {
        const std::complex<double> mu = adi.shifts.values[c.cyc % adi.shifts.values.size()];
        ar.shifts.push_back(mu);
        coef.push_back(-2.0 * mu.real());
        ++c.cyc; ++c.iters_host;
    }
    keepRpk.push_back(Rpk.buf);
    mark(4);
}

void DenseStep::enqueue_single_chunk(const Compressed& cz, Chain& c, const Chunk& ck) {
    const int nit = ck.nit, base_it = ck.base_it;
    const size_t rpd = c.rpd;
    const bool use_pk = c.use_pk;
    const Mat& R = cz.R;
    const Mat& Rring = ck.Rring;
    const Mat& Gm = c.Gm;
    if (!co.single_built) { co.build_single(ctx); co.single_built = true; }
    AdiFastArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = n; a.k = k; a.nstrip = c.nstrip; a.kst = c.kst; adi_fast_pick(n, k, &a.mode, &a.nt);
    DevArr<double> Rpk(ctx, use_pk ? rpd * (size_t)(nit + 1) : 1);
    const double* slot0 = c.Rp0.p;                        // first chunk: packed by the init launch
    if (use_pk && base_it > 0) { adi_fast_pack_r(ctx, n, k, R.p, R.ld, Rpk.p, st.p); slot0 = Rpk.p; }
    a.T = cz.Tm.p; a.ldt = cz.Tm.ld; a.tdiag = 0; a.alpha = 1.0; a.st = st.p; a.nws = c.nws.p;
    a.chain_timed = 1; a.do_strips = 1; a.G_prev = Gm.p;
    double by1 = 0.0, fl1 = 0.0;
    adi_fast_cost(a, &by1, &fl1);
    {
        TimedScope chain_ts(ctx, "adi_fast_iter", by1 * nit, fl1 * nit, nit + 2);   // the two flush launches ride along (riders only)
        for (int j = 1; j <= nit; ++j) {
            const std::complex<double> mu = adi.shifts.values[c.cyc % adi.shifts.values.size()];
            a.Apack = co.pack[c.cyc % co.pack.size()];
            if (j == 1) { a.Rcur = R.p; a.ldr = R.ld; } else { a.Rcur = Rring.p + (size_t)(j - 2) * k * Rring.ld; a.ldr = Rring.ld; }
            a.Rnext = Rring.p + (size_t)(j - 1) * k * Rring.ld; a.ldr_next = Rring.ld;
            a.Rpc = use_pk ? (j == 1 ? slot0 : Rpk.p + (size_t)(j - 1) * rpd) : nullptr;
            a.Rpn = use_pk ? Rpk.p + (size_t)j * rpd : nullptr;
            Mat Vj = Vall.colsview(c.vcols_used + (j - 1) * k, k);
            a.V = Vj.p; a.ldv = Vj.ld;
            a.two_mu = 2.0 * mu.real();
            const int g = base_it + j;
            a.G_prev = j >= 2 ? Gm.p + (size_t)((g - 1) & 1) * k * k : nullptr;
            a.G_prev2 = j >= 3 ? Gm.p + (size_t)((g - 2) & 1) * k * k : nullptr;
            a.it_prev2 = g - 2; a.do_strips = 1;
            adi_fast_iter(ctx, a);
            ar.shifts.push_back(mu);
            coef.push_back(-2.0 * mu.real());
            ++c.cyc; ++c.iters_host;
        }
        const int g = base_it + nit;
        a.do_strips = 0; a.Apack = nullptr; a.Rnext = nullptr; a.V = nullptr;
        a.Rpc = use_pk ? Rpk.p + (size_t)nit * rpd : nullptr; a.Rpn = nullptr;
        a.Rcur = Rring.p + (size_t)(nit - 1) * k * Rring.ld; a.ldr = Rring.ld;
        a.G_prev = Gm.p + (size_t)(g & 1) * k * k;
        a.G_prev2 = nit >= 2 ? Gm.p + (size_t)((g - 1) & 1) * k * k : nullptr;
        a.it_prev2 = g - 1;
        adi_fast_iter(ctx, a);
        a.G_prev = nullptr;
        a.G_prev2 = Gm.p + (size_t)(g & 1) * k * k;
        a.it_prev2 = g;
        adi_fast_iter(ctx, a);
    }
    mark(4);
}

// Control block (header + the norms of this chunk), tolerances and the SMW breakdown flag in ONE read-back.  The update
//   X <- X + sum_j (-2 mu_j) V_j T V_j'      (adi.jl:166-174 accumulated: one batched product + one GEMM)
// of this chunk is enqueued right behind the read-back kernel: how many of the speculatively enqueued iterations count is
// read from the control block ON THE DEVICE (DevCount), so the device works on X while the host waits for the words.
// false: the probe rejected the warm basis (the solve ended before its first iteration).
bool DenseStep::fetch_chunk(Compressed& cz, Chain& c, const Chunk& ck, const bool use_warm) {
    const int base_it = ck.base_it, nit = ck.nit;
    {
        const size_t stb = sizeof(int) * 4 + sizeof(double) * (2 + (size_t)std::min(512, base_it + nit + 1 + 8));
        long long serr8 = 0;
        std::function<void()> between;
        if (c.specx) between = [&]() {
            DevCount dc{st.p, base_it, nit, k};
            Mat Wc(ctx, n, k * nit);
            std::vector<GemmBatchDesc> descs;
            for (int j = 0; j < nit; ++j) {
                Mat Vj = Vall.colsview(c.vcols_used + j * k, k), Wj = Wc.colsview(j * k, k);
                const double cj = -2.0 * adi.shifts.values[(ck.cyc0 + (size_t)j) % adi.shifts.values.size()].real();
                descs.push_back({Vj.p, cz.Tm.p, Wj.p, nullptr, cj, n, k, k, Vj.ld, cz.Tm.ld, Wj.ld, 0});
            }
            DevCount dcb = dc; dcb.per = 1;
            gemm_batched(ctx, descs, "gemm_xupdate", dcb);
            Mat Vch = Vall.colsview(c.vcols_used, k * nit);
            gemm_sym_update(ctx, Wc, Vch, sx.X, "gemm_xupdate", dc);
        };
        ctx_fetch_overlap(ctx, between, st.p, stb, &sx.land->st, tols.p, 12 * sizeof(double), sx.land->tols, m ? (const void*)co.serr8.p : nullptr, m ? 8 : 0, &serr8);
        sx.land->serr = (int)serr8;
    }
    h = sx.land->st;
    if (use_warm && base_it == 0 && sx.trace.warm)
        std::fprintf(stderr, "[warm] step %d basis %d -> launch width %d, J = %d, missed^2 %.2e, dropped^2 %.2e, tol^2 %.2e %s  (Jacobi: %.4f sweeps.rounds, set-up %.1f us, sweeps %.1f us = %.0f cycles)\n", sx.dense_steps + 1, sx.q_cols, k,
                     (int)sx.land->tols[4], sx.land->tols[6], sx.land->tols[7], sx.land->tols[1] * sx.land->tols[1], sx.land->tols[5] != 0.0 ? "REJECTED" : "accepted",
                     sx.land->tols[3], sx.land->tols[8], sx.land->tols[9], sx.land->tols[10]);
    if (use_warm && base_it == 0 && sx.land->tols[5] != 0.0) return false;
    const int acc_it = std::min(std::max(h.iters - base_it, 0), nit);
    for (int j = 1; j <= acc_it; ++j) { ar.norms.push_back(h.norms[(base_it + j) & 511]); ar.norm_iters.push_back(base_it + j); }
    if (base_it == 0) init_norm = h.norms[0];
    if (!c.specx && acc_it > 0) c.any_plain = true;
    c.iters_host = base_it + acc_it;
    c.vcols_used += acc_it * k;
    c.cyc = c.cyc - nit + acc_it;
    ar.shifts.resize(c.iters_host); coef.resize(c.iters_host);
    if (acc_it > 0) cz.R = ck.Rring.colsview((acc_it - 1) * k, k);
    if (h.done || acc_it < nit || c.iters_host >= adi.maxiters) c.finished = true;
    return true;
}

// chunks whose update was not enqueued during the read-back (more than 48 iterations at once): all increments in one go
void DenseStep::late_x_update(const Compressed& cz) {
    Wall = Mat(ctx, n, k * acc_total);
    std::vector<GemmBatchDesc> descs;
    for (int j = 0; j < acc_total; ++j) {
        Mat Vj = Vall.colsview(j * k, k), Wj = Wall.colsview(j * k, k);
        descs.push_back({Vj.p, cz.Tm.p, Wj.p, nullptr, coef[j], n, k, k, Vj.ld, cz.Tm.ld, Wj.ld, 0});
    }
    gemm_batched(ctx, descs, "gemm_xupdate");
    Mat Vacc = Vall.colsview(0, k * acc_total);
    gemm_sym_update(ctx, Wall, Vacc, sx.X, "gemm_xupdate");
}

// the factor of this step's residual is the next step's basis
void DenseStep::next_basis(const Compressed& cz, const bool use_warm) {
    if (!use_warm) {
        if (sx.eig_state == 2) { sx.eig_state = 0; sx.qcur = -1; }        // (a rejected warm step: the next cold factor gets a fresh eigenbasis)
    } else if (cz.wnext >= 0 && k > 0) {
        sx.qcur = cz.wnext; sx.q_cols = cz.wq_next;
        sx.warm_J = std::max(0, std::min(k, (int)sx.land->tols[4]));
        const double t2 = sx.land->tols[1] * sx.land->tols[1];
        sx.est_ratio = t2 > 0.0 ? sx.land->tols[6] / t2 : -1.0;
        ar.rhs_cols = sx.warm_J;
    } else sx.qcur = -1;
}

// the solve's record, and the feedback of the new X:  P1 = E' X,  K' = P1 B      (lowrank_ros1.jl:53-56)
void DenseStep::close() {
    sx.dense_steps++;
    ar.abstol = sx.land->tols[0];
    ar.iters = acc_total;
    ar.initial_norm = k > 0 ? init_norm : 0.0;
    ar.res_norm = k > 0 ? (acc_total > 0 ? h.res_norm : init_norm) : 0.0;
    ar.norms.insert(ar.norms.begin(), ar.initial_norm); ar.norm_iters.insert(ar.norm_iters.begin(), 0);
    ar.converged = ar.res_norm <= ar.abstol;
    if (!ar.converged) ar.warnings |= 1;
    sx.hint = acc_total;
    cache->iters_hint = acc_total;
    mark(5);
    spmm(ctx, P, P.valEt.p, sx.X, sx.P1, 1.0, 0.0, nullptr, &sx.P1t);
    Mat Kt(ctx, n, m);
    gemm_thin(ctx, false, n, m, n, 1.0, sx.P1.p, sx.P1.ld, prob.B.p, prob.B.ld, 0.0, Kt.p, Kt.ld);
    sx.Kt = Kt;
    mark(6);
}

// One Ros1 step on the dense state, phase by phase.  Returns false (state untouched) when the fast chain cannot take the step.
// DESIGN.md ("The dense-X step: phases and enqueue order") lists what must not move between the streams and threads.
bool ros1_dense_step(Ctx* ctx, const GdreProblem& prob, const GaleOperator& op_base, double tau, const AdiOptions& adi, FactorCache* cache, DenseXState& sx,
                     AdiResult& ar, bool more_steps) {
    DRE_REQUIRE(sx.land != nullptr, "pinned host memory unavailable");
    DenseStep s(ctx, prob, op_base, tau, adi, cache, sx, ar, more_steps);
    s.mark(0);
    s.side.begin();
    s.assemble_residual();
    s.adopt_eigenbasis();
    const bool warm = s.warm_try();
    s.st = DevArr<AdiState>(ctx, 1);
    int rc = 1;
    if (warm) { rc = s.attempt(true); if (rc == 1) sx.warm_rejected++; else if (rc == 0) sx.warm_used++; }
    if (rc == 1) rc = s.attempt(false);
    if (rc != 0) return false;
    s.close();
    s.side.finish(op_base);
    return true;
}

std::shared_ptr<DenseXState> dense_x_new(Ctx* ctx, SideWorker* worker) { return std::make_shared<DenseXState>(ctx, worker); }
const Mat& dense_x_X(const DenseXState& sx) { return sx.X; }
const Mat& dense_x_Kt(const DenseXState& sx) { return sx.Kt; }
void dense_x_report(DenseXState& sx) { sx.trace.report(); }

void dense_x_start(Ctx* ctx, const GdreProblem& prob, DenseXState& sx, const LDLt& X, const Mat& Kt, int hint) {
    const Pencil& P = *prob.P;
    const int n = P.n, c = X.rank();
    sx.X = Mat(ctx, n, n);
    if (c > 0) {
        Mat Lcat(ctx, n, c), LD(ctx, n, c);
        hcat_scale_blocks(ctx, X, Lcat, LD);
        gemm(ctx, false, true, 1.0, LD, Lcat, 0.0, sx.X, nullptr, "gemm_xupdate");
        symmetrize(ctx, sx.X);
    } else fill_mat(ctx, sx.X, 0.0);
    sx.P1 = Mat(ctx, n, n);
    sx.P1t = Mat(ctx, n, n);
    spmm(ctx, P, P.valEt.p, sx.X, sx.P1, 1.0, 0.0, nullptr, &sx.P1t);
    sx.Kt = Kt;
    sx.hint = hint;
}

// K(t) is complete and nothing downstream of the LDL' form of the last X feeds it: with final_x_lazy the result takes a handle of the
// dense matrix (shared with sx: the buffer stays out of the pool for as long as the result lives) and the band reduction — a host-paced
// chain of ~70 short kernels — runs when a caller asks for that X (gdre_result_x), if one ever does
LDLtP dense_x_final(Ctx* ctx, DenseXState& sx, double ctf, bool steps_on, GdreResult& out) {
    if (steps_on) DRE_HIP(hipStreamSynchronize(ctx->stream));          // (the stamp below starts behind the last step's trailing kernels)
    const auto f0 = std::chrono::steady_clock::now();
    LDLtP X;
    if (ctx->final_x_lazy) {
        out.final_x = std::make_shared<FinalXDense>();
        out.final_x->ctx = ctx; out.final_x->Xd = sx.X; out.final_x->ctf = ctf;
    } else X = dense_to_ldlt(ctx, sx.X.rows, sx.X, ctf);
    if (steps_on)
        std::fprintf(stderr, "[final X, us] %.0f (%s)\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - f0).count(),
                     ctx->final_x_lazy ? "kept dense: factored on demand" : "dense_to_ldlt");
    return X;
}

LDLtP dense_to_ldlt(Ctx* ctx, int n, const Mat& Xd, double ctf) {
    Mat I(ctx, n, n), D(ctx, n, n);
    set_identity(ctx, I, 1.0);
    copy_mat(ctx, Xd, D);
    LDLtP X = ldlt_make(ctx, n, I, D, 1.0, false);
    ldlt_compress(ctx, *X, ctf, false);
    return X;
}

}  // namespace dre

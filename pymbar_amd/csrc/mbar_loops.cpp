// The solve entry points of libmbar_hip.so, the pure self-consistent iteration (pymbar/mbar_solvers.py:231-242 in a loop) and what
// the solver loops share.  The adaptive loops themselves: mbar_loop_device.cpp, mbar_loop_host.cpp.
#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

namespace mbar {
namespace host {

// ---- shared by the loops ---------------------------------------------------------------------------
int enter_solve(mbar_ctx* c, const double* f_inout, const char* who, Ld0Guard& guard, double* t0) {
    if (c && c->ext_base) return ext_holds_rows_only(c, who);
    if (!c || !f_inout) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (!c->have_Nk) return fail(c, MBAR_ERR_STATE, "mbar_ctx_set_Nk has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    *t0 = now_ms();
    guard.c = c;
    c->ld0_valid = false;
    return refresh_poison(c);
}

// (or the ranks wait for each other in different all-reduces.  A collective itself: every rank calls it at the same point whatever
// its local outcome)
int agree_all_ok(mbar_ctx* c, bool& ok) {
    if (c->nranks <= 1) return MBAR_OK;
    double v = ok ? 0.0 : 1.0;
    int rc = allreduce_host(c, &v, 1, 1);
    if (rc) return rc;
    ok = !(v > 0.0);
    return MBAR_OK;
}

int capture_batch(mbar_ctx* c, hipGraphExec_t* exec, int64_t batch, const std::function<int(int64_t)>& enqueue) {
    hipGraph_t graph = nullptr;
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int crc = MBAR_OK;
    for (int64_t b = 0; b < batch && crc == MBAR_OK; ++b) crc = enqueue(b);
    hipError_t ee = hipStreamEndCapture(c->stream, &graph);
    if (crc) return crc;
    if (ee != hipSuccess) return fail(c, MBAR_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
    ee = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ee != hipSuccess) return fail(c, MBAR_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ee));
    return MBAR_OK;
}

int debug_stamps(mbar_ctx* c, long long** out) {
    *out = nullptr;
    if (!std::getenv("MBAR_DEBUG_STAMPS")) return MBAR_OK;
    if (!c->stamps) HIPCHK(c, hipMalloc((void**)&c->stamps, STAMP_WORDS * sizeof(long long)));
    HIPCHK(c, hipMemsetAsync(c->stamps, 0, STAMP_WORDS * sizeof(long long), c->stream));
    *out = c->stamps;
    return MBAR_OK;
}

// ---- self-consistent loop: plan -> start -> run -> harvest ------------------------------------------
// Everything the loop decides once per solve (plan_sci fills it; nothing changes it afterwards).
struct SciPlan {
    int64_t rows = 0, na = 0;  // rows swept; entries of aden on the device (the larger of rows and Kp)
    int64_t batch = 0;         // iterations of a full batch ("sci_batch")
    int nbk = 0, first = 0;    // 16-state row blocks; gauge state
    bool fast = false;         // the register-tiled sweeps (else run_lse's generic path)
    bool merged = false;       // update and sweep of an iteration in ONE launch (k_sci_small)
    bool use_graph = false;    // full-size batches replay a captured hipGraph
    LaunchGeom g;
    int64_t graph_sig = 0;
    uint32_t live = 0;         // (merged) SciLoopArgs::live: the row pairs that hold a state with samples
};

// The plan of one solve -- and every allocation of it: geometry and buffers are fixed for the whole solve (nothing may allocate
// inside a capture, nothing is resized with work in flight).
int plan_sci(mbar_ctx* c, int64_t maxiter, SciPlan& p) {
    const int64_t K = c->K, Kp = c->Kp;
    const int64_t rows = p.rows = lse_rows(c);
    p.na = std::max(rows, Kp);
    p.batch = c->opt_sci_batch;
    p.first = c->sampled[0];
    p.fast = use_fast(c);
    p.nbk = (int)(rows / 16);
    LaunchGeom& g = p.g;
    if (p.fast) g = lse_geometry(p.nbk, 1, c->num_cu, (c->N + TS - 1) / TS, c->opt_grid, lse_variant_for(c));
    g.balanced = c->opt_small_balanced ? 1 : 0;
    const bool one_rank = c->nranks <= 1 && !c->comm;
    // Few states on one rank ("sci_merged", default): update and sweep of an iteration in ONE launch (k_sci_small) -- the update of
    // iteration i rides in the prologue of the sweep at f_i, so an iteration is one kernel instead of sweep + single-workgroup
    // update (config 2: ~9 us of a 62 us iteration).  Records / state double-buffered by the parity of the iteration, which the
    // captured batch bakes in: batches must be even.
    p.merged = p.fast && g.variant == 4 && c->opt_sci_merged && one_rank && !stream_transport(c) && rows == Kp && p.batch % 2 == 0;
    if (p.merged)  // (cannot change during a solve)
        for (int64_t j = 0; j < rows / 2; ++j)
            if ((2 * j < K && c->Nk[2 * j] > 0.0) || (2 * j + 1 < K && c->Nk[2 * j + 1] > 0.0)) p.live |= 1u << j;
    // Launch-bound regime (a K=32, N=1e6 sweep is ~60 us): capture a whole batch into a hipGraph and replay it.
    p.use_graph = p.fast && c->opt_graph && one_rank && maxiter >= p.batch;  // (no per-kernel events inside a graph)
    p.graph_sig = ((int64_t)g.blocks << 32) ^ ((int64_t)g.variant << 24) ^ (p.merged ? (1 << 16) : 0) ^ (g.balanced ? (1 << 17) : 0) ^
                  (c->opt_sci_pingpong ? (1 << 18) : 0) ^ p.first;
    HIPCHK(c, c->f_hist.grow((size_t)256 * Kp));
    int rc = ensure_red(c, (size_t)rows + 8);
    if (!rc && p.fast) rc = ensure(c, c->part, std::max((size_t)g.nwaves * (rows + 1), (size_t)2 * g.blocks * rows + g.blocks));
    if (!rc && p.fast) rc = ensure(c, c->scratch, ((size_t)g.nwaves / 32 + 16) * (rows + 1));
    return rc;
}

// The SCI loop's counterpart of BatchSchedule (mbar_loop_device.cpp).  Nothing to look at without the convergence test: the batches
// go out back to back and only the last one is read.  With it: the first batch has the standard size (a captured graph), every
// later one the number of iterations the relative change -- it decays geometrically -- still needs to reach `tol`, from its last
// two values (rows and changes of up to 256 iterations are kept, the first one below `tol` is the answer whatever was enqueued
// behind it).  A look costs ~70 us of idle device (config 2: 92 iterations in two looks instead of six).
// delta[0 .. nb): the relative changes of the batch just read; `batch` when they do not predict (or the solve is done).
int64_t sci_next_batch(const double* delta, int64_t nb, double tol, int64_t batch, bool done) {
    int64_t want = batch;
    if (!done && nb >= 2) {
        const double d1 = delta[nb - 1], d0 = delta[nb - 2];
        if (d1 > tol && d0 > d1 && d1 > 0.0) {
            const double left = std::log(d1 / tol) / std::log(d0 / d1);
            if (left == left) want = (int64_t)std::min(254.0, std::ceil(left)) + 2;
        }
    }
    return std::max<int64_t>(2, std::min<int64_t>(256, want + (want & 1)));  // (even: records and state alternate by parity)
}

// MBAR_DEBUG_STAMPS: the stamps of the last k_sci_small launch (10 ns units relative to the workgroup's first stamp)
int dump_sci_small_stamps(mbar_ctx* c) {
    long long st[24];
    HIPCHK(c, hipMemcpy(st, c->stamps, sizeof(st), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[mbar] k_sci_small workgroup 0, end of the tile loop per wave (us):");
    for (int w = 0; w < 8; ++w) std::fprintf(stderr, " %.2f", (st[16 + w] - st[0]) * 0.01);
    std::fprintf(stderr, "\n");
    for (int w = 0; w < 2; ++w) {
        const long long* p = st + 8 * w;
        std::fprintf(stderr, "[mbar] k_sci_small workgroup %s (us since its start; start offset to workgroup 0: %.2f): tables %.2f, update done %.2f, first tile in %.2f, "
                     "sweep done %.2f, barrier %.2f, record written %.2f\n", w ? "mid" : "0", (p[0] - st[0]) * 0.01, (p[1] - p[0]) * 0.01, (p[2] - p[0]) * 0.01,
                     (p[3] - p[0]) * 0.01, (p[4] - p[0]) * 0.01, (p[5] - p[0]) * 0.01, (p[6] - p[0]) * 0.01);
    }
    return MBAR_OK;
}

// The loop proper: what one iteration enqueues, the graph of a full batch, the batches, and the results back.
struct SciLoop {
    mbar_ctx* c;
    const SciPlan& p;
    const double tol;
    const int64_t K, Kp;
    std::vector<double> hf, ha;  // f at the last accepted iterate (until then: the start point); aden at the start point
    long long* stamps = nullptr;
    int64_t it = 0;              // iterations accepted so far
    bool converged = false;
    double last_delta = std::numeric_limits<double>::quiet_NaN();

    SciLoop(mbar_ctx* c_, const SciPlan& p_, double tol_, const double* f_start)
        : c(c_), p(p_), tol(tol_), K(c_->K), Kp(c_->Kp), hf((size_t)c_->Kp, 0.0), ha((size_t)p_.na) {
        std::copy(f_start, f_start + K, hf.begin());
        build_aden(c, f_start, ha.data(), p.na);
    }

    // f and aden of the start point on the device
    int upload_start() {
        HIPCHK(c, hipMemcpyAsync(d_f(c), hf.data(), Kp * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_aden(c), ha.data(), p.na * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MBAR_OK;
    }
    // iteration 0 of the merged loop: the plain sweep at the start point leaves its records and f in the parity-0 buffers
    int prime_merged() {
        HIPCHK(c, hipMemcpyAsync(c->scratch, hf.data(), p.rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
        ScopedTimer t(c, MBAR_TIMER_LSE);
        HIPCHK(c, launch_lse(c->stream, p.nbk, 1, p.g, c->u, c->ld, c->N, d_aden(c), c->cw, nullptr, nullptr, nullptr, c->part,
                             c->part + (size_t)2 * p.g.blocks * p.rows));
        return MBAR_OK;
    }
    int start() {
        int rc = upload_start();
        if (rc || !p.merged) return rc;
        rc = prime_merged();
        return rc ? rc : debug_stamps(c, &stamps);
    }

    SciLoopArgs merged_args(int64_t b) const {
        SciLoopArgs q;
        q.Nk = d_Nk(c);
        q.lnNk = d_lnNk(c);
        q.K = (int)K;
        q.first = p.first;
        q.tol = tol;
        q.state = c->scratch;
        q.rec = c->part;
        q.nrec = p.g.blocks;
        q.f_hist = c->f_hist + (size_t)b * Kp;
        q.delta_out = d_delta(c) + b;
        q.parity = (int)((it + b + 1) & 1);
        q.live = p.live;
        q.balanced = p.g.balanced;
        q.pingpong = c->opt_sci_pingpong ? 1 : 0;
        q.stamps = stamps;
        return q;
    }

    // One SCI iteration into history slot b: sweep -> level-1 reduction -> [all-reduce] -> update (which folds the last reduction
    // level in); merged: the one launch that does both.
    int enqueue_iteration(int64_t b, bool timed) {
        const int64_t rows = p.rows;
        const LaunchGeom& g = p.g;
        if (!p.fast) {
            int rc = run_lse(c, 1, rows, nullptr, nullptr, false);
            if (!rc) rc = allreduce_dev(c, c->red, rows, 0);
            if (rc) return rc;
        } else {
            ScopedTimer t(c, MBAR_TIMER_LSE, timed);
            if (p.merged) {
                HIPCHK(c, launch_sci_small(c->stream, p.nbk, g, c->u, c->ld, c->N, c->cw, merged_args(b)));
                return MBAR_OK;
            }
            HIPCHK(c, launch_lse(c->stream, p.nbk, 1, g, c->u, c->ld, c->N, d_aden(c), c->cw, nullptr, nullptr, nullptr, c->part,
                                 c->part + (size_t)g.nwaves * rows));
        }
        const double* upd_src = p.fast ? c->part.p : c->red.p;
        int64_t upd_n = p.fast ? g.nwaves : 1;
        // the update kernel sums the partial records itself, 256 / KW of them in parallel per state (KW = states
        // rounded up to a power of two): worth it up to ~32 sequential adds per thread, a level-1 reduction otherwise
        int64_t kw2 = 1;
        while (kw2 < std::min<int64_t>(rows, 256)) kw2 <<= 1;
        if (p.fast && (int64_t)g.nwaves * kw2 > 8192) {
            HIPCHK(c, launch_reduce_level1(c->stream, c->part, g.nwaves, rows, c->scratch, &upd_n));
            upd_src = c->scratch;
        }
        if (p.fast && (c->nranks > 1 || c->comm)) {
            HIPCHK(c, launch_reduce(c->stream, upd_src, upd_n, rows, c->scratch + (size_t)upd_n * rows, c->red));
            int rc = allreduce_dev(c, c->red, rows, 0);
            if (rc) return rc;
            upd_src = c->red;
            upd_n = 1;
        }
        HIPCHK(c, launch_sci_update(c->stream, upd_src, upd_n, rows, d_Nk(c), d_lnNk(c), K, p.na, p.first, tol, d_f(c), d_aden(c),
                                    c->f_hist + (size_t)b * Kp, d_delta(c) + b));
        return MBAR_OK;
    }

    // The captured graph of one full batch, kept on the context across solves
    int prepare_graph() {
        if (c->sci_graph && c->sci_graph_batch == p.batch && c->sci_graph_sig == p.graph_sig && c->sci_graph_tol == tol) return MBAR_OK;
        if (c->sci_graph) HIPCHK(c, hipGraphExecDestroy(c->sci_graph));
        c->sci_graph = nullptr;
        int rc = enqueue_iteration(0, false);  // eager warm-up: sets kernel attributes outside the capture
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        rc = upload_start();  // (the warm-up moved f and aden)
        if (rc) return rc;
        rc = capture_batch(c, &c->sci_graph, p.batch, [this](int64_t b) { return enqueue_iteration(b, false); });
        if (rc) return rc;
        c->sci_graph_batch = p.batch;
        c->sci_graph_sig = p.graph_sig;
        c->sci_graph_tol = tol;
        return MBAR_OK;
    }

    // Batches between two looks at the host (sci_next_batch) until an iterate is below `tol` or `maxiter` is reached
    int run(int64_t maxiter, int check_convergence) {
        int rc = p.use_graph ? prepare_graph() : MBAR_OK;
        if (rc) return rc;
        std::vector<double> hdelta(256), hrows;
        int64_t next_nb = p.batch;
        while (it < maxiter && !converged) {
            const int64_t nb = std::min(next_nb, maxiter - it);
            if (p.use_graph && nb == p.batch) {
                HIPCHK(c, hipGraphLaunch(c->sci_graph, c->stream));
            } else {
                for (int64_t b = 0; b < nb; ++b) {
                    rc = enqueue_iteration(b, c->opt_timing != 0);
                    if (rc) return rc;
                }
            }
            if (!check_convergence && it + nb < maxiter) {
                it += nb;
                continue;
            }
            hrows.resize((size_t)nb * Kp);
            HIPCHK(c, hipMemcpyAsync(hdelta.data(), d_delta(c), nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(hrows.data(), c->f_hist, (size_t)nb * Kp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            rc = sync_stream(c);
            if (rc) return rc;
            int64_t stop = nb;  // index within the batch of the accepted iterate
            if (check_convergence) {
                for (int64_t b = 0; b < nb && !converged; ++b)
                    if (std::isnan(hdelta[b]) || hdelta[b] < tol) {
                        stop = b + 1;
                        converged = true;
                    }
                double ctl[3] = {(double)stop, converged ? 1.0 : 0.0, (double)sci_next_batch(hdelta.data(), nb, tol, p.batch, converged)};
                rc = agree_with_rank0(c, ctl, 3);
                if (rc) return rc;
                stop = (int64_t)(ctl[0] + 0.5);
                converged = ctl[1] > 0.5;
                next_nb = (int64_t)(ctl[2] + 0.5);
            }
            it += stop;
            last_delta = hdelta[stop - 1];
            std::copy(hrows.begin() + (size_t)(stop - 1) * Kp, hrows.begin() + (size_t)stop * Kp, hf.begin());
        }
        return MBAR_OK;
    }

    // Results back: f of the states with samples, the counters
    int harvest(double* f_inout, mbar_solve_result& res) {
        if (stamps) {
            int rc = dump_sci_small_stamps(c);
            if (rc) return rc;
        }
        for (int64_t k = 0; k < K; ++k)
            if (c->Nk[k] > 0.0) f_inout[k] = hf[k];
        if (converged) res.success = 1;
        res.iterations = res.sci_iter = it;
        res.max_delta = last_delta;
        return MBAR_OK;
    }
};

// The device-resident loop while it serves, the host-driven loop for the rest
int run_adaptive(mbar_ctx* c, std::vector<double>& f, double tol, int64_t maxiter, int64_t min_sc_iter, double gamma, int check_convergence,
                 double* history, int64_t history_rows, mbar_solve_result& res, std::vector<double>& psum, double& max_delta, bool& on_device) {
    on_device = device_loop_eligible(c) && !c->u_poison && f_is_finite(c, f.data(), 1) && maxiter > 0;
    int rc, handbacks = 0;
    while (on_device) {
        bool handed_back = false;
        rc = adaptive_device_loop(c, f, tol, maxiter, min_sc_iter, gamma, check_convergence, history, history_rows, res, psum,
                                  max_delta, handed_back);
        if (rc) return rc;
        if (!handed_back) break;
        // The device handed the solve back.  A step too large for the sweeps' anchor point is a one-off (typically the
        // first Newton step from a poor start): ONE host-driven iteration, then back to the device, which re-anchors at
        // the new f.  Anything else (Newton system not positive definite, non-finite candidate) stays on the host.
        // (a non-finite candidate is usually the same situation seen from the other side -- a state whose weights
        // underflow at the current f -- and the host iteration handles it in log space; a Newton system that is not
        // positive definite, or repeated hand-backs, stay on the host)
        const int reason = c->h_ctl[CTL_REASON];
        const bool one_off = (reason == 2 || reason == 3) && ++handbacks <= 6 && res.iterations + 1 < maxiter;
        if (!one_off) {
            on_device = false;
            break;
        }
        rc = adaptive_host_loop(c, f, tol, res.iterations + 1, min_sc_iter, gamma, check_convergence, history, history_rows, res,
                                psum, max_delta);
        if (rc) return rc;
        if (res.success || !f_is_finite(c, f.data(), 1)) break;
    }
    if (!on_device && !res.success && res.iterations < maxiter)
        return adaptive_host_loop(c, f, tol, maxiter, min_sc_iter, gamma, check_convergence, history, history_rows, res, psum, max_delta);
    return MBAR_OK;
}

}  // namespace host
}  // namespace mbar

extern "C" {

int mbar_solve_adaptive(mbar_ctx* c, double* f_inout, double tol, int64_t maxiter, int64_t min_sc_iter, double gamma,
                        int check_convergence, double* history, int64_t history_rows, mbar_solve_result* result) {
    Ld0Guard guard;
    double t0;
    int rc = enter_solve(c, f_inout, "mbar_solve_adaptive", guard, &t0);
    if (rc) return rc;
    const int64_t K = c->K;
    std::vector<double> f(f_inout, f_inout + K), psum;
    mbar_solve_result res;
    std::memset(&res, 0, sizeof(res));
    double max_delta = std::numeric_limits<double>::quiet_NaN();
    bool on_device = false;
    rc = run_adaptive(c, f, tol, maxiter, min_sc_iter, gamma, check_convergence, history, history_rows, res, psum, max_delta, on_device);
    if (rc) return rc;
    double gn = 0.0;
    if ((int64_t)psum.size() == K)
        for (int k : c->sampled) gn += (psum[k] - c->Nk[k]) * (psum[k] - c->Nk[k]);
    res.gnorm = std::sqrt(gn);
    c->last_psum = (int64_t)psum.size() == K ? psum : std::vector<double>();
    res.max_delta = max_delta;
    res.wall_ms = now_ms() - t0;
    if (std::getenv("MBAR_DEBUG_TIMING") && res.iterations > 0)
        std::fprintf(stderr, "[mbar] adaptive: %lld iterations, %.3f ms per iteration (%s loop)\n", (long long)res.iterations,
                     res.wall_ms / res.iterations, on_device ? "device-resident" : "host-driven");
    std::copy(f.begin(), f.end(), f_inout);
    if (result) *result = res;
    return MBAR_OK;
}

int mbar_ctx_last_solve_psum(mbar_ctx* c, double* psum_out) {
    if (!c || !psum_out) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if ((int64_t)c->last_psum.size() != c->K) return fail(c, MBAR_ERR_STATE, "no adaptive solve has left its per-state sums on this context");
    std::copy(c->last_psum.begin(), c->last_psum.end(), psum_out);
    return MBAR_OK;
}

int mbar_solve_sci(mbar_ctx* c, double* f_inout, double tol, int64_t maxiter, int check_convergence,
                   mbar_solve_result* result) {
    Ld0Guard guard;
    double t0;
    int rc = enter_solve(c, f_inout, "mbar_solve_sci", guard, &t0);
    if (rc) return rc;
    mbar_solve_result res;
    std::memset(&res, 0, sizeof(res));
    if (unusable(c, f_inout)) {  // NaN in, NaN out; isnan(max_delta) counts as converged (:636)
        for (int64_t k = 0; k < c->K; ++k)
            if (c->Nk[k] > 0.0) f_inout[k] = std::numeric_limits<double>::quiet_NaN();
        res.success = 1;
        res.max_delta = std::numeric_limits<double>::quiet_NaN();
        if (result) *result = res;
        return MBAR_OK;
    }
    SciPlan p;
    rc = plan_sci(c, maxiter, p);
    if (rc) return rc;
    SciLoop loop(c, p, tol, f_inout);
    rc = loop.start();
    if (!rc) rc = loop.run(maxiter, check_convergence);
    if (!rc) rc = loop.harvest(f_inout, res);
    if (rc) return rc;
    res.wall_ms = now_ms() - t0;
    if (result) *result = res;
    return MBAR_OK;
}

}  // extern "C"

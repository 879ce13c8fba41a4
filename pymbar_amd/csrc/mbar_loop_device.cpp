// The device-resident adaptive loop of libmbar_hip.so (adaptive(), pymbar/mbar_solvers.py:510-667, with nothing but eight control
// words per batch crossing to the host): plan -> start -> upload -> run -> harvest.
#include "mbar_ctx.h"

namespace mbar {
namespace host {

// Device-resident loop: one iteration = {Gram sweep, reduction, [all-reduce], k_newton, two-candidate sweep, reduction,
// [all-reduce], k_select}, enqueued back to back (or replayed from a hipGraph in batches); f, the candidates, the choice
// and the convergence test never leave the device, and the host reads eight control words per batch.  Iterations
// enqueued past convergence are no-ops (every kernel looks at CTL_DONE first).
bool device_loop_eligible(const mbar_ctx* c) {
    if (!c->opt_device_loop || !use_fast(c)) return false;
    if (c->nranks > 1 && !stream_transport(c)) return false;  // the host transport needs the host in the loop
    const int64_t ntiles = (c->N + TS - 1) / TS;
    const LaunchGeom gl = lse_geometry((int)(c->Kp / 16), 2, c->num_cu, ntiles, c->opt_grid, lse_variant_for(c));
    // 129 .. 256 states: the one-read Gram kernel, the four-waves-per-CU evaluation kernel and the blocked Cholesky solve
    if (c->Kp > 128) return c->opt_device_loop_wide && use_quad(c) && gl.variant == 5;
    return gl.variant == 1;
}

inline size_t ad_off_f() { return 0; }
inline size_t ad_off_psum(const mbar_ctx* c) { return (size_t)c->Kp; }
inline size_t ad_off_cand(const mbar_ctx* c) { return (size_t)2 * c->Kp; }
inline size_t ad_off_ratio(const mbar_ctx* c) { return (size_t)4 * c->Kp; }
inline size_t ad_off_prm(const mbar_ctx* c) { return (size_t)5 * c->Kp; }
inline size_t ad_off_state(const mbar_ctx* c) { return (size_t)5 * c->Kp + 4; }
inline size_t ad_off_hist(const mbar_ctx* c) { return (size_t)5 * c->Kp + 8; }

int ensure_ad(mbar_ctx* c, int64_t hist_rows) {
    const int64_t cap = std::max<int64_t>(1024, std::min<int64_t>(hist_rows, 1 << 20));
    if (!c->ad || c->ad_hist_cap < cap) {
        int rc = drop_graphs(c);
        if (rc) return rc;
        HIPCHK(c, c->ad.grow(ad_off_hist(c) + (size_t)4 * cap));
        c->ad_hist_cap = cap;
    }
    HIPCHK(c, c->ad_ints.grow((size_t)(CTL_WORDS + c->Kp)));
    HIPCHK(c, c->h_ctl.grow((size_t)CTL_WORDS));
    return MBAR_OK;
}

// Everything the device-resident loop decides once per solve (plan_device_loop fills it; nothing changes it afterwards).
struct DeviceLoopPlan {
    int m = 0, nb = 0;        // states with samples, 16-state row blocks
    bool wide = false;        // 129 .. 256 states: the one-read kernels whose four waves share a tile stream
    bool pmode = false;       // the sweeps run on the resident probability matrix
    bool fused = false;       // ... and ONE sweep per iteration gives the gradients and the (speculated) next Gram matrix
    bool light = false;       // last iteration without its Gram matrix (CTL_LIGHT)
    bool unit = false;        // k_fused without the x 1.0 work of unit multiplicities
    bool merged = false;      // the Newton solve rides in the launch of the previous iteration's selection (k_select_newton)
    bool warm = false;        // the kept probability matrix serves: start with one fused sweep instead of the build
    bool use_graph = false;   // full-size batches replay a captured hipGraph
    LaunchGeom gg, gl, gp, gb;  // Gram sweep, main sweep, the plain sweep standing in for the fused one, build sweep
    size_t rec_g = 0, rec_l = 0, off_gram = 0;  // doubles per Gram record / per-state record; offset of the Gram blocks in `red`
    LoopCtl lc_slot, lc_flat;   // kernels reading the slot the control words name / a flat vector
    int64_t batch = 0, graph_sig = 0;
    std::vector<double> an0, cm0;  // aden at the start point; (warm) its multipliers exp(an0 - a0) relative to the anchor of P
};

// The plan of one solve: modes, launch geometries, record sizes -- and every allocation of the solve, which happens here and
// nowhere else.  The ranks agree on each outcome before the first sweep: a rank that could not get its buffers (or its resident
// probability matrix) must not wander off into a different sequence of collectives than its peers.  FOUR collectives
// (agree_all_ok), in this order, each called by every rank whatever its local outcome:
//   1. P fits (else: classic sweeps everywhere)   2. `light`   3. the buffers are allocated (else: the solve fails everywhere)
//   4. `warm`
// An error of a collective returns at once; a local allocation error returns after the third.
int plan_device_loop(mbar_ctx* c, const std::vector<double>& f, int check_convergence, const double* history, int64_t history_rows,
                     DeviceLoopPlan& p) {
    const int64_t Kp = c->Kp;
    const int64_t ntiles = (c->N + TS - 1) / TS;
    const int nb = p.nb = (int)(Kp / 16);
    p.m = (int)c->sampled.size();
    // P mode: the sweeps run on the resident probability matrix (one more K x N array); if it does not fit ON ANY RANK, every rank
    // runs the classic sweeps on u.
    const bool wide = p.wide = Kp > 128;
    // (129 .. 256 states: P mode exists in its fused form only)
    bool pmode = c->opt_pmode && !c->P_failed && (!wide || (c->opt_wide_pmode && c->opt_fused));
    int arc = ensure_ad(c, history ? history_rows : 0);
    if (!arc && wide && c->chol.grow(NEWTON_CHOL_WORK) != hipSuccess)
        arc = fail(c, MBAR_ERR_HIP, "allocation of the Newton workspace failed");
    // (a new P is zeroed below, once the buffers are sized: nothing of this call is queued before that.  A return before the fill
    // gives the block back: a P that stays is one that has been zeroed)
    struct FreshP {
        mbar_ctx* c;
        bool pending;
        ~FreshP() { if (pending) c->P.reset(); }
        operator bool() const { return pending; }
    } zero_p{c, false};
    if (!arc && pmode && !c->P) {
        arc = drop_graphs(c);
        if (!arc) {
            zero_p.pending = c->P.grow((size_t)Kp * c->ld) == hipSuccess;
            if (!zero_p) {
                (void)hipGetLastError();
                c->P_failed = true;
                pmode = false;
            }
        }
    }
    {
        bool p_ok = pmode;
        int rc = agree_all_ok(c, p_ok);
        if (rc) return rc;
        if (pmode && !p_ok) {  // a peer has no room for its P: classic sweeps everywhere (this rank keeps its array for later)
            pmode = false;
            c->error = "resident probability matrix does not fit on every rank: classic sweeps";
        }
    }
    p.pmode = pmode;
    if (!arc && pmode && c->pm_vec.grow((size_t)3 * Kp) != hipSuccess)
        arc = fail(c, MBAR_ERR_HIP, "allocation of the P-mode vectors failed");
    const bool fused = p.fused = pmode && c->opt_fused;
    // (fused loop: the Newton solve of an iteration rides in the launch of the previous iteration's selection -- k_select_newton --
    // so the loop proper is four launches per iteration (+ the idle stand-in sweep of light_last); a solve of its own is needed at
    // the start and after a pause)
    p.merged = fused && !wide && c->opt_merge_select;
    // Last iteration without its Gram matrix (CTL_LIGHT, mbar_internal.h): an idle launch per iteration against ONE lighter sweep per
    // solve.  Worth it where the fused sweep is bound by the matrix cores and the plain one by HBM -- 65 states and more (K = 128:
    // 1.9 ms against 3.1 at config 3; at 64 states and fewer both are HBM-bound and nothing is gained) -- and from ~5e7 matrix
    // entries per rank on (a sweep of ~0.13 ms); option light_last = 2 drops both bounds.
    // (129 .. 256 states: the one-read fused sweep has an evaluation-only body of its own and needs no stand-in launch)
    bool light = fused && check_convergence && c->opt_light_last != 0 &&
                 (c->opt_light_last >= 2 || (nb >= 5 && (double)Kp * (double)c->N >= 5.0e7));
    // geometry and buffers are fixed for the whole solve (nothing may allocate inside a capture)
    LaunchGeom& gg = p.gg;
    LaunchGeom& gl = p.gl;
    LaunchGeom& gp = p.gp;
    gg = wide ? gram_quad_geometry(nb, c->num_cu, ntiles, c->opt_grid) : gram_geometry(nb * 16, true, c->num_cu, ntiles, c->opt_grid);
    p.unit = !c->weighted && !c->opt_fused_general;
    gl = fused ? fused_geometry(nb, c->num_cu, ntiles, c->opt_grid, p.unit)
         : pmode ? psweep_geometry(nb, c->num_cu, ntiles, c->opt_grid)
                 : lse_geometry(nb, 2, c->num_cu, ntiles, c->opt_grid, lse_variant_for(c));
    if (wide) gg.live_blocks = gl.live_blocks = quad_live_blocks(c);
    if (fused) {  // the separate Gram sweep (when it runs) leaves its partial records where the fused sweep leaves them
        gg.blocks = gl.blocks;
        gg.nwaves = gl.nwaves;
    }
    // the plain sweep that stands in for the fused one leaves ITS per-state records where the fused sweep leaves them too: as many
    // waves as the fused grid has, in workgroups of the plain sweep's size
    gp = psweep_geometry(wide ? 8 : nb, c->num_cu, ntiles, 0);
    if (light && !wide && gl.nwaves % gp.waves != 0) light = false;
    if (light && !wide) {
        gp.blocks = gl.nwaves / gp.waves;
        gp.nwaves = gp.psum_records = gl.nwaves;
    }
    {
        bool l_ok = light;  // (every rank derives it from its own shard length: agree, like every decision that changes what is launched)
        int rcl = agree_all_ok(c, l_ok);
        if (rcl) return rcl;
        light = light && l_ok;
    }
    p.light = light;
    // build sweep of P mode: with the fused loop it also accumulates the Gram matrix at the anchor (grid of the fused sweep)
    const LaunchGeom& gb = p.gb = fused ? build_gram_geometry(nb, c->num_cu, ntiles, c->opt_grid)
                                        : build_sweep_geometry(nb, c->num_cu, ntiles, c->opt_grid);
    const size_t rec_g = p.rec_g = (size_t)nb * (nb + 1) / 2 * 256;
    const size_t rec_l = p.rec_l = (size_t)2 * Kp;
    const size_t off_gram = p.off_gram = rec_l + 2;
    if (!arc) arc = ensure_red(c, off_gram + rec_g);
    if (!arc)
        arc = ensure(c, c->part,
                     std::max(std::max((size_t)gg.nwaves * rec_g, (size_t)gl.nwaves * (rec_l + 2)), (size_t)gb.nwaves * Kp));
    // (level-1 scratch of the widest reduction: the fused loop reduces the per-state sums and the Gram records in ONE pair of launches)
    if (!arc)
        arc = ensure(c, c->scratch,
                     std::max(((size_t)std::max(gg.nwaves, gl.nwaves) / 32 + 1) * (rec_g + rec_l + 2), ((size_t)gb.nwaves / 32 + 1) * (Kp + rec_g)));
    if (!arc && c->weighted && !c->lden_eff) arc = fail(c, MBAR_ERR_STATE, "weighted context without its logden buffer");
    if (!arc && fused) arc = ensure(c, c->part_g, (size_t)gl.nwaves * rec_g);
    if (!arc && zero_p) {
        if (launch_zero(c->stream, c->P, (size_t)Kp * c->ld * sizeof(double)) == hipSuccess) zero_p.pending = false;
        else arc = fail(c, MBAR_ERR_HIP, "zero fill of P failed");
    }
    {
        bool ok = arc == MBAR_OK;
        const std::string local_err = c->error;
        int rc = agree_all_ok(c, ok);
        if (rc) return rc;
        if (arc) return arc;
        if (!ok) return fail(c, MBAR_ERR_STATE, "a peer rank could not allocate its solver buffers");
        c->error = local_err;
    }
    p.lc_slot.ctl = p.lc_flat.ctl = c->ad_ints;
    p.lc_slot.slot_stride = c->ld;
    p.lc_slot.unclamped = p.lc_flat.unclamped = c->u_checked && !c->u_posinf;
    p.lc_slot.pmode = p.lc_flat.pmode = pmode;
    // Only full-size batches replay a captured hipGraph (see BatchSchedule); the graph is kept across solves and rebuilt when
    // anything that shapes a launch has changed
    p.batch = c->opt_adapt_batch;
    p.use_graph = c->opt_graph && !stream_transport(c);
    p.graph_sig = ((int64_t)gg.blocks << 40) ^ ((int64_t)gl.blocks << 20) ^ ((int64_t)p.m << 12) ^ (pmode ? 128 : 0) ^ (fused ? 256 : 0) ^
                  (c->weighted ? 64 : 0) ^ (p.lc_slot.unclamped ? 512 : 0) ^ (p.merged ? 1024 : 0) ^ (light ? 2048 : 0) ^ (int64_t)nb;
    // Warm start: the resident probability matrix of an earlier solve on this matrix is still there and the start point lies
    // inside the window of its anchor -- the per-state sums, the reciprocals and the Gram matrix at f come from ONE fused sweep
    // (both multiplier rows = exp(aden(f) - a0)) instead of the build sweep (16 K N bytes of traffic and K N exponentials).
    p.an0.assign((size_t)Kp, 0.0);
    p.cm0.assign((size_t)Kp, 0.0);
    build_aden(c, f.data(), p.an0.data(), Kp);
    bool warm = fused && c->opt_pcache && c->P_valid && (int64_t)c->P_a0.size() == Kp;
    for (int64_t k = 0; warm && k < Kp; ++k) {
        const bool live = !std::isinf(p.an0[k]), was = !std::isinf(c->P_a0[k]);
        if (live != was) warm = false;
        else if (live) {
            const double d = p.an0[k] - c->P_a0[k];
            if (!(std::fabs(d) < 200.0)) warm = false;
            p.cm0[k] = std::exp(d);
        }
    }
    int rc = agree_all_ok(c, warm);
    if (rc) return rc;
    p.warm = warm;
    return MBAR_OK;
}

// ---- start: f's per-state sums in `psum`, the slot vector(s) and (fused loop) the first Hessian's reduced Gram blocks on the device.
// Initial gradient (mbar_solvers.py:570), four ways:

// Classic: the evaluation sweep, logden(f) stays in slot 0.
int start_classic(mbar_ctx* c, const DeviceLoopPlan&, const std::vector<double>& f, std::vector<double>& psum, mbar_solve_result&) {
    return eval_core(c, f.data(), 1, 0, c->logden[0], nullptr, psum.data(), nullptr, nullptr);
}

// Warm: ONE fused sweep on the kept P, both multiplier rows = cm0.
int start_warm(mbar_ctx* c, const DeviceLoopPlan& p, const std::vector<double>&, std::vector<double>& psum, mbar_solve_result& res) {
    const int64_t K = c->K, Kp = c->Kp;
    std::vector<int> z((size_t)CTL_WORDS, 0);  // slot 0, running: the sweep leaves the reciprocals of its first row in slot 1
    HIPCHK(c, hipMemcpyAsync(c->ad_ints, z.data(), z.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    std::copy(p.cm0.begin(), p.cm0.end(), c->hstage.p);
    std::copy(p.cm0.begin(), p.cm0.end(), c->hstage + Kp);
    HIPCHK(c, hipMemcpyAsync(d_aden(c), c->hstage, (size_t)2 * Kp * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->red, 0, p.off_gram * sizeof(double), c->stream));
    {
        ScopedTimer t(c, MBAR_TIMER_OTHER);
        HIPCHK(c, launch_fused(c->stream, p.nb, p.gl, c->P, c->ld, c->N, d_aden(c), c->cw, c->weighted ? c->cwsq : c->cw, p.unit,
                               c->logden[0], c->part_g, c->part, p.lc_slot));
    }
    HIPCHK(c, launch_reduce2(c->stream, c->part, (int64_t)p.rec_l, c->part_g, (int64_t)p.rec_g, p.gl.nwaves, c->scratch, c->red,
                             c->red + p.off_gram));
    int rc = allreduce_dev(c, c->red, (int64_t)(p.off_gram + p.rec_g), 0);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->hred, c->red, (size_t)Kp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    rc = sync_stream(c);
    if (rc) return rc;
    for (int64_t k = 0; k < K; ++k) psum[k] = c->hred[k] * p.cm0[k];  // (the sweep returns the sums without the multipliers)
    res.warm_starts += 1;
    return MBAR_OK;
}

// Build, 129 .. 256 states (fused loop only): the probability matrix from plain sweeps -- evaluation at the anchor (log-denominators
// into slot 1, per-state sums), then P = exp(a0 - u - logden) and the Gram matrix at the anchor; 1 / s = 1 in slot 0.
int start_build_wide(mbar_ctx* c, const DeviceLoopPlan& p, const std::vector<double>& f, std::vector<double>& psum, mbar_solve_result& res) {
    c->P_valid = false;
    int rc = eval_core(c, f.data(), 1, 0, c->logden[1], nullptr, psum.data(), nullptr, nullptr);
    if (rc) return rc;
    if (!c->weighted) {
        // unweighted: the Gram sweep at the anchor forms exactly P as its operands -- it writes them out on the way (one sweep
        // instead of make-P + Gram-from-P: 8 K N bytes read + 8 K N written once)
        ScopedTimer t(c, MBAR_TIMER_OTHER);
        HIPCHK(c, launch_gram_quad(c->stream, p.nb, p.gg, c->u, c->ld, c->N, d_aden(c), c->logden[1], c->part_g, LoopCtl(), c->P));
        HIPCHK(c, launch_reduce(c->stream, c->part_g, p.gg.nwaves, (int64_t)p.rec_g, c->scratch, c->red + p.off_gram));
        rc = allreduce_dev(c, c->red + p.off_gram, (int64_t)p.rec_g, 0);
        if (rc) return rc;
        HIPCHK(c, launch_fill(c->stream, c->logden[0], 1.0, c->ld));
    } else {
        // weighted: make-P, then the Gram matrix from P with unit reciprocals (each operand carries sqrt(c_n))
        {
            ScopedTimer t(c, MBAR_TIMER_OTHER);
            HIPCHK(c, launch_make_p(c->stream, c->num_cu, c->u, c->ld, c->N, c->Kp, d_aden(c), c->logden[1], c->P));
            HIPCHK(c, launch_fill(c->stream, c->logden[0], 1.0, c->ld));
        }
        HIPCHK(c, launch_rinv_weighted(c->stream, c->logden[0], c->cw, c->N, c->lden_eff));
        LoopCtl lp;
        lp.pmode = true;
        {
            ScopedTimer t(c, MBAR_TIMER_GRAM);
            HIPCHK(c, launch_gram_quad(c->stream, p.nb, p.gg, c->P, c->ld, c->N, d_anum(c), c->lden_eff, c->part_g, lp));
        }
        HIPCHK(c, launch_reduce(c->stream, c->part_g, p.gg.nwaves, (int64_t)p.rec_g, c->scratch, c->red + p.off_gram));
        rc = allreduce_dev(c, c->red + p.off_gram, (int64_t)p.rec_g, 0);
        if (rc) return rc;
    }
    rc = sync_stream(c);
    if (rc) return rc;
    c->P_a0 = p.an0;
    c->P_valid = true;
    res.builds += 1;
    return MBAR_OK;
}

// `len` doubles per record of `part` reduced into red + off, all-reduced, and on the host in hred + off when this returns
int reduce_to_host(mbar_ctx* c, const double* part, int64_t nrec, int64_t len, size_t off) {
    HIPCHK(c, launch_reduce(c->stream, part, nrec, len, c->scratch, c->red + off));
    int rc = allreduce_dev(c, c->red + off, len, 0);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->hred + off, c->red + off, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

// Build, up to 128 states: ONE sweep writes P = exp(a0 - u - logden(a0)) with a0 = aden(f) and leaves 1 / s = 1 in slot 0; in the
// fused loop it accumulates the first Hessian's Gram matrix as well (its reduced blocks wait in `red` for k_newton).
int start_build_narrow(mbar_ctx* c, const DeviceLoopPlan& p, const std::vector<double>& f, std::vector<double>& psum, mbar_solve_result& res) {
    const int64_t K = c->K, Kp = c->Kp;
    c->P_valid = false;
    build_aden(c, f.data(), c->hstage, Kp);
    HIPCHK(c, hipMemcpyAsync(d_aden(c), c->hstage, (size_t)Kp * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->red, 0, p.off_gram * sizeof(double), c->stream));
    {
        ScopedTimer t(c, MBAR_TIMER_OTHER);
        if (p.fused)
            HIPCHK(c, launch_build_gram(c->stream, p.nb, p.gb, c->u, c->ld, c->N, d_aden(c), c->weighted ? c->cwsq : c->cw,
                                        c->weighted || !p.lc_slot.unclamped, c->P, c->logden[0], c->part_g));
        else
            HIPCHK(c, launch_build_sweep(c->stream, p.nb, p.gb, c->u, c->ld, c->N, d_aden(c), c->cw, c->P, c->logden[0], c->part));
    }
    if (p.fused) {
        // the Gram matrix at the anchor: one reduction, ONE all-reduce; the per-state sums are its row sums (the rows of p sum to
        // one: sum_n c_n p_kn = sum_j G_kj), taken on the host from the reduced blocks -- the build sweep accumulates none
        int rc = reduce_to_host(c, c->part_g, p.gb.nwaves, (int64_t)p.rec_g, p.off_gram);
        if (rc) return rc;
        gram_row_sums(c->hred + p.off_gram, p.nb, K, psum.data());
    } else {
        int rc = reduce_to_host(c, c->part, p.gb.nwaves, Kp, 0);
        if (rc) return rc;
        for (int64_t k = 0; k < K; ++k) psum[k] = c->hred[k];
    }
    c->P_a0 = p.an0;
    c->P_valid = true;
    res.builds += 1;
    return MBAR_OK;
}

// ---- solver state to the device: f, psum, the parameters, the control words, the sampled-state list, anum = aden(f), and (P mode)
// the anchor with the multipliers of f relative to it.  `res` carries the counters of the iterations already executed.
int upload_state(mbar_ctx* c, const DeviceLoopPlan& p, const std::vector<double>& f, const std::vector<double>& psum, double tol,
                 int64_t min_sc_iter, double gamma, int check_convergence, const mbar_solve_result& res) {
    const int64_t K = c->K, Kp = c->Kp;
    std::vector<double> h(ad_off_hist(c), 0.0);
    for (int64_t k = 0; k < K; ++k) {
        h[ad_off_f() + k] = f[k];
        h[ad_off_psum(c) + k] = psum[k];
    }
    h[ad_off_prm(c) + 0] = gamma;
    h[ad_off_prm(c) + 1] = tol;
    h[ad_off_prm(c) + 2] = (double)std::min<int64_t>(min_sc_iter, 1 << 30);
    h[ad_off_prm(c) + 3] = check_convergence ? 1.0 : 0.0;
    h[ad_off_state(c)] = std::numeric_limits<double>::quiet_NaN();
    std::vector<int> hi((size_t)CTL_WORDS + Kp, 0);
    // two-sweep loops and the classic mode run a Gram sweep per iteration; the fused loop starts with the Gram matrix
    // its build sweep accumulated (multipliers cgram = 1 at the anchor)
    hi[CTL_NEEDGRAM] = p.fused ? 0 : 1;
    hi[CTL_GRAMSWEEPS] = 0;
    hi[CTL_SPEC] = 1;
    hi[CTL_SLOT] = p.warm ? 1 : 0;
    hi[CTL_ITER] = (int)res.iterations;
    hi[CTL_SCI] = (int)res.sci_iter;
    hi[CTL_NR] = (int)res.nr_iter;
    for (int i = 0; i < p.m; ++i) hi[CTL_WORDS + i] = c->sampled[i];
    HIPCHK(c, hipMemcpyAsync(c->ad, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ad_ints, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_anum(c), p.an0.data(), p.an0.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    std::vector<double> pv;
    if (p.pmode) {  // anchor point a0 (= aden(f) after a build), multipliers of the current f relative to it (1 after a build)
        pv.assign((size_t)3 * Kp, 1.0);
        std::copy(c->P_a0.begin(), c->P_a0.end(), pv.begin());
        for (int64_t k = 0; k < Kp; ++k) {
            if (p.warm) pv[(size_t)Kp + k] = pv[(size_t)2 * Kp + k] = p.cm0[k];
            if (!(k < K && c->Nk[k] > 0.0)) pv[(size_t)Kp + k] = pv[(size_t)2 * Kp + k] = 0.0;
        }
        HIPCHK(c, hipMemcpyAsync(c->pm_vec, pv.data(), pv.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MBAR_OK;
}

// The kernel arguments of k_newton / k_select / k_select_newton: where the state uploaded above lives
int make_adapt_args(mbar_ctx* c, const DeviceLoopPlan& p, AdaptArgs& q) {
    const int64_t Kp = c->Kp;
    q.gram_red = c->red + p.off_gram;
    q.lse_red = c->red;
    q.f = c->ad + ad_off_f();
    q.psum = c->ad + ad_off_psum(c);
    q.cand = c->ad + ad_off_cand(c);
    q.ratio = c->ad + ad_off_ratio(c);
    q.aden = d_aden(c);
    q.anum = d_anum(c);
    q.Nk = d_Nk(c);
    q.lnNk = d_lnNk(c);
    q.sampled = c->ad_ints + CTL_WORDS;
    q.m = p.m;
    q.K = (int)c->K;
    q.Kp = (int)Kp;
    q.ctl = c->ad_ints;
    q.prm = c->ad + ad_off_prm(c);
    q.state = c->ad + ad_off_state(c);
    q.hist = c->ad + ad_off_hist(c);
    q.hist_cap = c->ad_hist_cap;
    q.pmode = p.pmode ? 1 : 0;
    q.a0 = c->pm_vec;
    q.ccur = p.pmode ? c->pm_vec + Kp : nullptr;
    q.fused = p.fused ? 1 : 0;
    q.cgram = p.fused ? c->pm_vec + 2 * Kp : nullptr;
    q.light_ok = p.light ? 1 : 0;
    q.newton_ldlt = c->opt_newton_ldlt ? 1 : 0;
    if (const char* e = std::getenv("MBAR_NEWTON_LDLT")) q.newton_ldlt = std::atoi(e) != 0 ? 1 : 0;
    return debug_stamps(c, &q.stamps);
}

// MBAR_DEBUG_STAMPS: the phase stamps k_select_newton left, one line per launch
int dump_select_newton_stamps(mbar_ctx* c) {
    std::vector<long long> st(STAMP_WORDS);
    HIPCHK(c, hipMemcpy(st.data(), c->stamps, st.size() * sizeof(long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < 64; ++i) {
        const long long* p = st.data() + 16 * i;
        if (!p[0] || !p[5]) continue;
        std::fprintf(stderr, "[mbar] k_select_newton launch %d (shader clocks): select %lld, set-up %lld, elimination %lld, solution %lld, candidates %lld, total %lld; of the elimination: pivot loops %lld, exchange + trailing update %lld; of the selection: inputs %lld, Gram staged %lld, matrix-vector product %lld, sums %lld, maxima %lld\n",
                     i, p[1] - p[0], p[2] - p[1], p[3] - p[2], p[4] - p[3], p[5] - p[4], p[5] - p[0], p[6], p[7], p[8] - p[0], p[9] - p[8], p[10] - p[9],
                     p[11] - p[10], p[12] - p[11]);
    }
    return MBAR_OK;
}

// Batches between two looks at the control words: 6, 2, 4, then `adapt_batch` (8) each.  Iterations enqueued past convergence
// (or past a pause of the fused loop) are no-ops of ~3.5 us per kernel; real solves take 5-8 iterations, and for the small
// problems pymbar is mostly used on two wasted iterations of a fixed batch of 8 were a tenth of the solve.  After a pause the
// batches restart at 1, 2, 4: a phase in which the self-consistent candidate keeps winning pauses every iteration.  Only
// full-size batches replay a captured hipGraph (eager launches are as fast at these kernel counts: the queue never runs
// dry), so a short solve never pays for a capture.
// (a fixed number of iterations -- no convergence test -- has nothing to look for early: full batches from the start, and up
// to four of them between two looks at the control words; a pause or a hand-back turns the rest into no-op launches as ever)
struct BatchSchedule {
    int64_t batch;
    bool fixed_count;
    int64_t nbatch = 0, ramp;  // ramp: cap on the batch size while recovering from a pause
    BatchSchedule(int64_t batch_, bool fixed_count_) : batch(batch_), fixed_count(fixed_count_), ramp(batch_) {}
    struct Round { int64_t want; int reps; };  // up to `reps` batches of `want` iterations before the next look
    Round next() {
        static const int64_t first_batches[3] = {6, 2, 4};
        const int64_t want = std::min(ramp, (nbatch < 3 && !fixed_count) ? std::min(batch, first_batches[nbatch]) : batch);
        ++nbatch;
        ramp = std::min(batch, ramp * 2);
        return {want, fixed_count && ramp == batch ? 4 : 1};
    }
    void paused() { ramp = 1; }
};

// The loop proper: what one iteration enqueues, the graph of a full batch, the batches, and the way back to the host.
struct DeviceLoop {
    mbar_ctx* c;
    const DeviceLoopPlan& p;
    AdaptArgs q;
    double* gram_part;  // partial records of the Gram matrix: the fused sweep's own array, else shared with the per-state records
    // The merged loop's Newton solve rides with the previous iteration's selection, so k_newton has a launch of its own only at
    // the start of the solve and after a pause: `need_newton` is raised there and taken by the next eager iteration or replay.
    // (the captured iterations are the steady-state ones: they never take it)
    bool need_newton = true;
    int64_t it, it_start;
    int32_t gram_sweeps = 0;
    bool converged = false, handed_back = false;

    DeviceLoop(mbar_ctx* c_, const DeviceLoopPlan& p_, int64_t it0)
        : c(c_), p(p_), gram_part(p_.fused ? c_->part_g : c_->part), it(it0), it_start(it0) {}
    bool take_need_newton() {
        const bool n = need_newton;
        need_newton = false;
        return n;
    }

    // Gram sweep at the current f with the known logden (the slot of the accepted candidate; P mode: the slots hold the
    // reciprocals 1 / s_n instead), reduced and all-reduced into the blocks k_newton reads.  Two-sweep loops: once per
    // iteration.  Fused loop: only after a pause (k_select found that the accepted candidate is not the one the sweep
    // speculated on) -- the host enqueues it, un-pausing first.
    int enqueue_gram(bool timed) {
        const double* lden = c->logden[0];
        LoopCtl lca = p.lc_slot;
        if (p.fused) HIPCHK(c, launch_ctl_resume(c->stream, c->ad_ints));
        if (c->weighted) {  // sum_n c_n p p^T: each operand carries sqrt(c_n), folded into the exponent / the reciprocal
            if (p.pmode)
                HIPCHK(c, launch_rinv_weighted(c->stream, c->logden[0], c->cw, c->N, c->lden_eff, p.lc_slot));
            else
                HIPCHK(c, launch_shift_logden(c->stream, c->logden[0], c->cw, 0.5, c->N, c->lden_eff, p.lc_slot));
            lden = c->lden_eff;
            lca = p.lc_flat;
        }
        {
            LaunchTimer t(c, MBAR_TIMER_GRAM, timed, lca);
            if (p.wide)
                HIPCHK(c, launch_gram_quad(c->stream, p.nb, p.gg, p.pmode ? c->P : c->u, c->ld, c->N, d_anum(c), lden, gram_part, lca));
            else
                HIPCHK(c, launch_gram_diag(c->stream, p.nb, p.gg, p.pmode ? c->P : c->u, c->ld, c->N, d_anum(c), lden, 0, gram_part,
                                           nullptr, lca));
        }
        HIPCHK(c, launch_reduce(c->stream, gram_part, p.gg.nwaves, (int64_t)p.rec_g, c->scratch, c->red + p.off_gram));
        if (stream_transport(c)) {
            int r2 = allreduce_dev(c, c->red + p.off_gram, (int64_t)p.rec_g, 0);
            if (r2) return r2;
        }
        return MBAR_OK;
    }

    // One iteration.  Fused loop: {k_newton, fused sweep, ONE reduction of its per-state sums and Gram records, ONE all-reduce
    // of both, k_select} -- the Gram matrix the next k_newton needs comes out of the same sweep as the gradients.  Two-sweep
    // loops: the Gram sweep first.  `own_newton`: the merged loop launches k_newton (the other forms always launch their solve).
    int enqueue_iteration(bool timed, bool own_newton) {
        // timing level 3: event pairs around the non-sweep sections too (the split that explains a multi-GPU iteration)
        const bool split = timed && c->opt_timing == 3;
        const bool solve = p.wide || !p.merged || own_newton;
        if (!p.fused) {
            int r2 = enqueue_gram(timed);
            if (r2) return r2;
        }
        {
            ScopedTimer sec(c, MBAR_TIMER_NEWTON, split && solve);
            if (p.wide)
                HIPCHK(c, launch_newton_chol(c->stream, q, c->chol));
            else if (solve)
                HIPCHK(c, launch_newton(c->stream, q));
        }
        double* psum_part = c->part;
        double* obj_part = c->part + (size_t)p.gl.nwaves * p.rec_l;
        {
            LoopCtl lcb = p.lc_slot;
            LaunchTimer t(c, p.fused ? MBAR_TIMER_FUSED : MBAR_TIMER_LSE, timed, lcb);
            if (p.fused) {
                HIPCHK(c, launch_fused(c->stream, p.nb, p.gl, c->P, c->ld, c->N, d_aden(c), c->cw, c->weighted ? c->cwsq : c->cw, p.unit,
                                       c->logden[0], gram_part, psum_part, lcb));
                if (p.light && !p.wide) {  // (idle unless k_newton found that this iteration is the last: then the fused sweep is the idle one)
                    LoopCtl lcl = p.lc_slot;
                    lcl.light_only = true;
                    HIPCHK(c, launch_psweep(c->stream, p.nb, 2, p.gp, c->P, c->ld, c->N, d_aden(c), c->cw, c->logden[0], nullptr, psum_part, lcl));
                }
            } else if (p.pmode)
                HIPCHK(c, launch_psweep(c->stream, p.nb, 2, p.gl, c->P, c->ld, c->N, d_aden(c), c->cw, c->logden[0], nullptr, psum_part,
                                        lcb));
            else
                HIPCHK(c, launch_lse(c->stream, p.nb, 2, p.gl, c->u, c->ld, c->N, d_aden(c), c->cw, c->logden[0], nullptr,
                                     nullptr, psum_part, obj_part, lcb));
        }
        int64_t ar_count = (int64_t)(p.rec_l + 2);
        {
            ScopedTimer sec(c, MBAR_TIMER_REDUCE, split);
            if (p.fused) {
                HIPCHK(c, launch_reduce2(c->stream, psum_part, (int64_t)p.rec_l, gram_part, (int64_t)p.rec_g, p.gl.nwaves, c->scratch, c->red,
                                         c->red + p.off_gram));
                ar_count = (int64_t)(p.off_gram + p.rec_g);
            } else if (p.pmode) {  // (no objective sums in P mode: the adaptive loop does not use them)
                HIPCHK(c, launch_reduce(c->stream, psum_part, p.gl.nwaves, (int64_t)p.rec_l, c->scratch, c->red));
            } else {
                HIPCHK(c, launch_reduce2(c->stream, psum_part, (int64_t)p.rec_l, obj_part, 2, p.gl.nwaves, c->scratch, c->red, c->red + p.rec_l));
            }
        }
        if (stream_transport(c)) {
            ScopedTimer sec(c, MBAR_TIMER_COMM, split);
            int r2 = allreduce_dev(c, c->red, ar_count, 0);
            if (r2) return r2;
        }
        {
            ScopedTimer sec(c, MBAR_TIMER_NEWTON, split);
            if (p.merged)
                HIPCHK(c, launch_select_newton(c->stream, q));
            else
                HIPCHK(c, launch_select(c->stream, q));
        }
        return MBAR_OK;
    }

    // The captured graph of one full batch of steady-state iterations, kept on the context across solves
    int prepare_graph() {
        if (c->ad_graph && c->ad_graph_batch == p.batch && c->ad_graph_sig == p.graph_sig) return MBAR_OK;
        if (c->ad_graph) HIPCHK(c, hipGraphExecDestroy(c->ad_graph));
        c->ad_graph = nullptr;
        // eager warm-up with the stop flag raised: every kernel is launched once outside the capture (function
        // attributes, module loading) and does nothing
        int one = 1;
        HIPCHK(c, hipMemcpyAsync(c->ad_ints + CTL_DONE, &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
        int rc = enqueue_iteration(false, false);
        if (rc) return rc;
        int zero = 0;
        HIPCHK(c, hipMemcpyAsync(c->ad_ints + CTL_DONE, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        rc = capture_batch(c, &c->ad_graph, p.batch, [this](int64_t) { return enqueue_iteration(false, false); });
        if (rc) return rc;
        c->ad_graph_batch = p.batch;
        c->ad_graph_sig = p.graph_sig;
        return MBAR_OK;
    }

    // Batches of iterations (BatchSchedule) until the control words say done, handed back, or `maxiter` is reached
    int run(int64_t maxiter, int check_convergence) {
        BatchSchedule sched(p.batch, !check_convergence);
        const bool timed = c->opt_timing != 0;
        bool done = false;
        int rc = MBAR_OK;
        while (it < maxiter && !done) {
            const BatchSchedule::Round round = sched.next();
            int64_t nbat = 0;
            for (int rep = 0; rep < round.reps && it + nbat < maxiter; ++rep) {
                const int64_t nb1 = std::min(round.want, maxiter - it - nbat);
                if (p.use_graph && nb1 == p.batch) {
                    rc = prepare_graph();
                    if (rc) return rc;
                    // (start of the solve / after a pause: the replayed iterations have no solve of their own)
                    if (take_need_newton() && p.merged) HIPCHK(c, launch_newton(c->stream, q));
                    HIPCHK(c, hipGraphLaunch(c->ad_graph, c->stream));
                } else {
                    for (int64_t b = 0; b < nb1; ++b) {
                        rc = enqueue_iteration(timed, take_need_newton());
                        if (rc) return rc;
                    }
                }
                nbat += nb1;
            }
            HIPCHK(c, hipMemcpyAsync(c->h_ctl, c->ad_ints, CTL_WORDS * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            rc = sync_stream(c);
            if (rc) return rc;
            const int64_t it_new = c->h_ctl[CTL_ITER];
            if (c->h_ctl[CTL_DONE] == 1) {
                converged = true;
                done = true;
            } else if (c->h_ctl[CTL_DONE] == 2) {
                handed_back = true;
                done = true;
            } else if (c->h_ctl[CTL_DONE] == 3) {
                // the fused loop paused itself after iteration it_new (the rest of the batch were no-ops): the accepted candidate's
                // Gram matrix has to be swept separately.  Every rank sees the same control words, so every rank comes by here.
                if (it_new <= it || it_new > it + nbat) return fail(c, MBAR_ERR_STATE, "device-resident adaptive loop lost count of its iterations");
                if (it_new < maxiter) {
                    rc = enqueue_gram(timed);
                    if (rc) return rc;
                    ++gram_sweeps;
                    sched.paused();
                    need_newton = true;  // (the solve that rode with the selection returned on the pause flag)
                }
            } else if (it_new != it + nbat) {
                return fail(c, MBAR_ERR_STATE, "device-resident adaptive loop lost count of its iterations");
            }
            it = it_new;
        }
        return MBAR_OK;
    }

    // Results back: f, psum, the history rows of the iterations that ran here, the counters, and why the loop handed back
    int harvest(std::vector<double>& f, std::vector<double>& psum, double* history, int64_t history_rows, mbar_solve_result& res,
                double& max_delta) {
        std::vector<double> h(ad_off_hist(c));
        HIPCHK(c, hipMemcpyAsync(h.data(), c->ad, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        // (only the rows of the iterations that ran HERE: after a hand-back the host loop wrote rows of its own in between)
        const int64_t row1 = history ? std::min<int64_t>(std::min<int64_t>(it, history_rows), c->ad_hist_cap) : 0;
        if (row1 > it_start)
            HIPCHK(c, hipMemcpyAsync(history + 4 * it_start, c->ad + ad_off_hist(c) + 4 * it_start, (size_t)(row1 - it_start) * 4 * sizeof(double),
                                     hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int64_t k = 0; k < c->K; ++k) {
            f[k] = h[ad_off_f() + k];
            psum[k] = h[ad_off_psum(c) + k];
        }
        if (it > it_start) max_delta = h[ad_off_state(c)];
        if (q.stamps) {
            int rc = dump_select_newton_stamps(c);
            if (rc) return rc;
        }
        if (converged) res.success = 1;
        res.iterations = it;
        res.sci_iter = c->h_ctl[CTL_SCI];
        res.nr_iter = c->h_ctl[CTL_NR];
        res.gram_sweeps += p.fused ? gram_sweeps : (int32_t)(it - it_start);
        res.light_sweeps += c->h_ctl[CTL_LIGHTS];
        if (p.fused && !p.wide && p.unit) res.fused_unit += 1;  // (what launch_fused was told: k_fused<.., UNIT>)
        if (handed_back) {
            c->P_valid = false;  // (the continuation re-anchors: a state whose weights underflow at this anchor has a zero row in P)
            static const char* why[] = {"", "the Newton system is not positive definite", "a candidate is too far from the point the sweeps are anchored at",
                                        "a candidate is not finite"};
            const int r = c->h_ctl[CTL_REASON];
            c->error = std::string("device-resident adaptive loop handed back to the host loop: ") + why[(r >= 1 && r <= 3) ? r : 0];
        }
        return MBAR_OK;
    }
};

// plan -> start -> upload -> run -> harvest.
// Returns MBAR_OK with handed_back = true when the loop stopped early for the host loop to continue (f, res updated).
int adaptive_device_loop(mbar_ctx* c, std::vector<double>& f, double tol, int64_t maxiter, int64_t min_sc_iter, double gamma,
                         int check_convergence, double* history, int64_t history_rows, mbar_solve_result& res,
                         std::vector<double>& psum, double& max_delta, bool& handed_back) {
    handed_back = false;
    c->ld0_valid = false;  // (the loop keeps reciprocals / rotating log-denominators in the slot vectors)
    psum.assign(c->K, 0.0);
    DeviceLoopPlan p;
    int rc = plan_device_loop(c, f, check_convergence, history, history_rows, p);
    if (rc) return rc;
    rc = !p.pmode ? start_classic(c, p, f, psum, res)
         : p.warm ? start_warm(c, p, f, psum, res)
         : p.wide ? start_build_wide(c, p, f, psum, res)
                  : start_build_narrow(c, p, f, psum, res);
    if (rc) return rc;
    rc = upload_state(c, p, f, psum, tol, min_sc_iter, gamma, check_convergence, res);
    if (rc) return rc;
    DeviceLoop loop(c, p, res.iterations);
    rc = make_adapt_args(c, p, loop.q);
    if (rc) return rc;
    rc = loop.run(maxiter, check_convergence);
    if (rc) return rc;
    rc = loop.harvest(f, psum, history, history_rows, res, max_delta);
    handed_back = loop.handed_back;
    return rc;
}
}  // namespace host
}  // namespace mbar
